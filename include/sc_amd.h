/*
 * sc_amd.h -- C ABI of libsc_amd.so: batched Paillier / DGK big-integer arithmetic on MI355X (gfx950).
 *
 * THIS header is what a maintainer binds: the context, key objects, the scheme operations (encrypt / randomize / decrypt /
 * is_zero), the protocol steps as five calls per batch, the random draws and the multi-GPU reassembly.  The primitives those are
 * composed of (modular products, the exponentiation shapes, inversion ...), the kernel-policy switches and the measurement
 * probes live in sc_amd_dev.h -- the toolbox of this repository's own tests, tools and bench, same library.
 *
 * The reference (TNO-MPC/protocols.secure_comparison 4.4.0) has NO native/FFI boundary: its hot path
 * is reached through the Python object API of the un-vendored scheme packages
 * (tno.mpc.encryption_schemes.{paillier,dgk,templates,utils}, pyproject.toml:32-38) by operator
 * overloading from Initiator.step_* / KeyHolder.step_*.  This header is therefore the boundary a
 * maintainer would bind with ctypes underneath those scheme objects; every entry point names the
 * reference call sites (file:line under /root/reference/src/tno/mpc/protocols/secure_comparison/,
 * "SC/") whose arithmetic it replaces.  INTEGRATION.md shows the ctypes stub.
 *
 * Conventions
 *   - Big integers are canonical residues stored as little-endian arrays of uint32_t words; a batch is
 *     a dense row-major array [count][nwords] in DEVICE memory (hipMalloc / sc_malloc / a torch tensor's
 *     data_ptr()).  "dptr" parameters are device pointers; "hptr" parameters are host pointers.
 *   - All functions return 0 on success or a negative sc_status; sc_last_error() gives the message.
 *   - Calls are asynchronous on the context's stream (sc_ctx_set_stream) unless stated otherwise.
 *   - No function falls back to host arithmetic: without a gfx950 device every call fails.
 *   - A context belongs to one host thread at a time and orders all its work on one stream; its temporary device buffers are
 *     reused from call to call.  sc_ctx_set_stream orders the work already queued on the previous stream before anything
 *     queued on the new one (event wait, no host synchronisation), so alternating streams on one context is safe; the
 *     caller's own input / output buffers follow the usual stream rules.  Use one context per GPU (one process per GPU under
 *     torch.distributed), or one per concurrent shard of a GPU.
 */
#ifndef SC_AMD_H
#define SC_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sc_ctx sc_ctx;

enum sc_status {
  SC_OK = 0,
  SC_ERR_ARG = -1,          /* bad argument (AssertionError / ValueError at the Python layer) */
  SC_ERR_HIP = -2,          /* HIP runtime error */
  SC_ERR_NOT_INVERTIBLE = -3, /* an element has no modular inverse (gmpy2/pow raise in the reference) */
  SC_ERR_UNSUPPORTED = -4,  /* modulus too large for the compiled configurations */
  SC_ERR_LAYOUT = -5        /* sc_keyholder_select_mult: a decrypted P exceeds the announced field layout (ValueError in Python) */
};

/* ---- context ------------------------------------------------------------------------------------ */
int sc_ctx_create(int device_id, sc_ctx** out_ctx);
void sc_ctx_destroy(sc_ctx* ctx);
int sc_ctx_set_stream(sc_ctx* ctx, void* hip_stream);   /* hipStream_t; NULL = default stream */
int sc_ctx_synchronize(sc_ctx* ctx);
const char* sc_last_error(sc_ctx* ctx);
/* The element named by the most recent SC_ERR_NOT_INVERTIBLE of this context (-1 before the first): the step-level entry points
 * have no bad_index parameter of their own. */
int64_t sc_last_bad_index(sc_ctx* ctx);
/* Bumped whenever an entry point is added, removed or changes meaning; the binding checks it (round 3: 3; round 4: 4 -- the header
 * split into sc_amd.h / sc_amd_dev.h, SC_STEP_DEFER_CHECKS and sc_ctx_check removed, sc_clock_probe and sc_ctx_policy added; round 5: 5
 * -- sc_ctx_set_pair_policy and sc_ctx_stats added in sc_amd_dev.h).  Still 5 with the selection entries (sc_initiator_select_d ..
 * sc_initiator_cx_finish, SC_ERR_LAYOUT): they are additions, nothing that was there changed. */
#define SC_ABI_VERSION 5
int sc_abi_version(void);
/* device memory helpers for callers that do not bring their own allocator */
int sc_malloc(sc_ctx* ctx, size_t bytes, void** out_dptr);
int sc_free(sc_ctx* ctx, void* dptr);
int sc_memcpy_h2d(sc_ctx* ctx, void* dptr, const void* hptr, size_t bytes);
int sc_memcpy_d2h(sc_ctx* ctx, void* hptr, const void* dptr, size_t bytes);

/* ---- scheme-level entry points: what the reference's scheme objects and protocol steps do, one call each ------------- */
/* A key object holds everything the scheme constructors derive ([ext] Paillier / DGK __init__; SC/keyholder.py:155-166): the
 * moduli N, N^2 (and p, p^2, q, q^2 for the key holder), the exponents N, lambda, p-1, q mod (p-1) .., mu / h_p / the CRT
 * recombination constants, g^-1, and the fixed-base tables for h.  With p / q (and v_p / v_q) the key is the key holder's and
 * -- unless SC_KEY_NO_CRT -- every exponentiation runs through CRT (identical integers, ~3.3x fewer limb products); without
 * them it is the public copy Alice receives (SC/initiator.py:177-203).  SC_KEY_NO_PAIRS forces exponentiations modulo N^2 to
 * use products modulo N^2 instead of the pair arithmetic modulo N (measurement / tests).  All arrays of the calls below are
 * device arrays of canonical words; N has `nwords` words, ciphertexts 2 * nwords; DGK residues `nwords` of its key. */
#define SC_KEY_NO_CRT 1
#define SC_KEY_NO_PAIRS 2
/* `flags` of the step entry points below.  SC_STEP_RANDOMIZERS_READY: the randomizer argument (rho_z / r_rand / rho3) holds the
 * FINISHED randomizers -- rho^N mod N^2 as [..][2 nwords(N)], h^r mod n as [..][nwords(n)] -- computed ahead of time by
 * sc_paillier_randomize / sc_dgk_randomize with c = NULL, e.g. on a second context and stream while the protocol's critical
 * path runs (the reference pre-generates its randomizers in background workers: boot_randomness_generation,
 * SC/initiator.py:205-210, SC/keyholder.py:174-179).  The step then applies them with one modular product each. */
#define SC_STEP_RANDOMIZERS_READY 1
/* Paillier key: the public modulus N and optionally the secret primes p, q (key holder) -- what `Paillier.from_security_parameter`
 * produces at SC/keyholder.py:155-158 and what the initiator receives as the public scheme (SC/initiator.py:177-203).  Every derived
 * modulus (N, N^2, p, q, p^2, q^2), exponent (N, lambda, p - 1, q - 1, q mod p - 1, ..), CRT constant and the pair contexts are
 * registered once; flags: SC_KEY_NO_CRT / SC_KEY_NO_PAIRS keep the literal single-modulus forms (tests, A/B).
 * Word counts: N^2 is always registered in 2 * nwords words, also where it is shorter (a 1025-bit N has 33 words, its 2049-bit N^2
 * 66, the top one zero in every ciphertext), and the kernel configuration follows the stored words, not the bit length alone: that
 * N^2 runs on (4,27), not on the (4,18) a 2049-bit modulus of 65 words would take.  p and q are both registered in
 * hw = nwords(max(bits(p), bits(q))) words and p^2, q^2 in 2 * hw: the shorter prime is padded, so the two CRT halves of a key always
 * run on the same kernel instances, whatever the difference in length. */
int sc_paillier_key_create(sc_ctx* ctx, const uint32_t* n_hptr, int nwords, const uint32_t* p_hptr /* nullable */,
                           const uint32_t* q_hptr /* nullable */, int pwords, int flags, int* out_key);
/* the primitive handles behind a key (for callers that mix scheme-level calls and the primitives of sc_amd_dev.h) */
int sc_paillier_key_mods(sc_ctx* ctx, int key, int* out_mod_n, int* out_mod_n2);
/* out[i] = 1 + m[i] N (negate: 1 - m[i] N) mod N^2: unsafe_encrypt(m, apply_encoding=False), SC/initiator.py:256, 562;
 * SC/keyholder.py:274-286. */
int sc_paillier_encrypt(sc_ctx* ctx, int key, const uint32_t* m_dptr, int m_words, int negate, uint32_t* out_dptr, uint64_t count);
/* ct.randomize() for a batch: out[i] = c[i] * rho[i]^N mod N^2 (c = NULL: the randomizers alone), rho: [count][nwords].
 * SC/initiator.py:109; SC/keyholder.py:126-128 (the key holder's goes through CRT over p^2, q^2). */
int sc_paillier_randomize(sc_ctx* ctx, int key, const uint32_t* c_dptr /* nullable */, const uint32_t* rho_dptr, uint32_t* out_dptr,
                          uint64_t count);
/* Paillier.decrypt(ct, apply_encoding=False): out[i] = L(c[i]^lambda mod N^2) mu mod N, [count][nwords] (SC/keyholder.py:195). */
int sc_paillier_decrypt(sc_ctx* ctx, int key, const uint32_t* c_dptr, uint32_t* out_dptr, uint64_t count);
/* The homomorphic sum of ciphertexts along one axis: c viewed as [outer][K][inner][2 nwords] canonical residues modulo N^2,
 * out[o][i] = prod_{j < K} c[o][j][i] mod N^2, [outer][inner][2 nwords] -- an encryption of the sum of the K plaintexts (mod N).  No
 * secret key, no randomness, no host round trip: sc_modprod_axis (sc_amd_dev.h) in the key's N^2 context, with its argument checks. */
int sc_paillier_sum_axis(sc_ctx* ctx, int key, const uint32_t* c_dptr, uint64_t outer, uint64_t K, uint64_t inner, uint32_t* out_dptr);
/* The running homomorphic sum along one axis, inclusive: out[o][j][i] = prod_{j' <= j} c[o][j'][i] mod N^2 in the shape of c -- an
 * encryption of the sum of the first j + 1 plaintexts.  sc_modscan_axis (sc_amd_dev.h) in the key's N^2 context, with its argument
 * checks; deterministic like sc_paillier_sum_axis, so re-randomize what is handed on. */
int sc_paillier_cumsum_axis(sc_ctx* ctx, int key, const uint32_t* c_dptr, uint64_t outer, uint64_t K, uint64_t inner, uint32_t* out_dptr);
/* A public linear map over ciphertexts along one axis: w_host [J][K] unsigned 64-bit weights on the host (free to reuse on return),
 * out[o][j][i] = prod_{k < K} c[o][k][i]^w[j][k] mod N^2, [outer][J][inner][2 nwords] -- an encryption of sum_k w[j][k] m[o][k][i]
 * (mod N).  sc_modlin_axis (sc_amd_dev.h) in the key's N^2 context, with its argument checks (K, J <= 1024, no zero size); deterministic
 * like sc_paillier_sum_axis, so re-randomize what is handed on.  Negative weights: negate the ciphertext (invert it modulo N^2). */
int sc_paillier_linear_axis(sc_ctx* ctx, int key, const uint32_t* c_dptr, uint64_t outer, uint64_t K, uint64_t inner, const uint64_t* w_host,
                            uint64_t J, uint32_t* out_dptr);
/* DGK key (`DGK.from_security_parameter`, SC/keyholder.py:161-166): public (n, g, h, u, t) and optionally secret (p, q, v_p, v_q); randomizer_bits = width of the exponent r of h^r ([ext]
 * ~2.5 t), window = fixed-base window of the tables for h, 1 .. 24 (2^window rows of the modulus's limb size per window: 6 GB
 * at 20, 82 GB at 24 for a 2048-bit n and 400-bit r; the key holder's half-size tables stop at 20).  table_src_ctx / table_src_key (nullable /
 * ignored): another context of the same GPU whose key of the same modulus, h, window and width already built the tables -- they
 * are shared read-only instead of built again (concurrent shard contexts; see sc_fbt_import). */
int sc_dgk_key_create(sc_ctx* ctx, const uint32_t* n_hptr, const uint32_t* g_hptr, const uint32_t* h_hptr, int nwords,
                      const uint32_t* u_hptr, int uwords, int t_bits, const uint32_t* p_hptr /* nullable */, const uint32_t* q_hptr,
                      int pwords, const uint32_t* vp_hptr, const uint32_t* vq_hptr, int vwords, int randomizer_bits, int window,
                      int flags, sc_ctx* table_src_ctx /* nullable */, int table_src_key, int* out_key);
int sc_dgk_key_info(sc_ctx* ctx, int key, int* out_mod_n, int* out_mod_p /* -1 without secret key */, uint64_t* out_table_bytes);
/* ct.randomize() for DGK: out[i] = c[i] * h^r[i] mod n (c = NULL: the randomizers alone); r: [count][ewords].
 * SC/keyholder.py:106-108 (CRT with exponents reduced modulo v_p, v_q), SC/initiator.py:153-154. */
int sc_dgk_randomize(sc_ctx* ctx, int key, const uint32_t* c_dptr /* nullable */, const uint32_t* r_dptr, int ewords,
                     uint32_t* out_dptr, uint64_t count);
/* unsafe_encrypt(bit) + .randomize() in one go: out[i] = g^bits[i] * h^r[i] mod n, bits: one byte per item
 * (SC/keyholder.py:213, 231 with :106-108). */
int sc_dgk_encrypt_bits_randomized(sc_ctx* ctx, int key, const uint8_t* bits_dptr, const uint32_t* r_dptr, int ewords,
                                   uint32_t* out_dptr, uint64_t count);
/* DGK.is_zero per ciphertext (SC/keyholder.py:249), and the whole of step 4j: any_flags[b] = OR over the planes of the bit-major
 * vector c[planes][inner][nwords] (:246-253). */
int sc_dgk_is_zero(sc_ctx* ctx, int key, const uint32_t* c_dptr, uint8_t* flags_dptr, uint64_t count);
int sc_dgk_any_zero(sc_ctx* ctx, int key, const uint32_t* c_dptr, int planes, uint64_t inner, uint64_t* any_flags_dptr);

/* Initiator.step_1 + step_3 + the plaintext side of 4c / 4e / 7 for a batch (SC/initiator.py:228-270, :289, :373, :558-562):
 * z = [[y]] [[x]]^-1 [[2^l + r]] mod N^2, randomized with rho_z^N when rho_z is given (:109); alpha = r mod 2^l,
 * alpha_tilde = (r - N) mod 2^l (flag rows, see FLAG ROWS below), rsmall = [r < (N-1)/2] (uint64), rshift = r div 2^l ([count][nwords]).
 * FLAG ROWS (every protocol step and plaintext helper): 1 <= l <= 255.  alpha, alpha_tilde and beta hold lw = ceil(l / 64)
 * little-endian uint64 words per comparison, laid out [count][lw], the bits above l zero; for l <= 64 that is one uint64 per
 * comparison.  rsmall, delta_a, dbit and delta_b are one uint64 per comparison at every l.  The plaintext helpers (sc_plain_alice /
 * sc_plain_bob and every step that runs them) additionally refuse l >= 32 nwords(N) with SC_ERR_ARG: 2^l + r must fit the
 * nwords(N) + 1 words of its output, and the protocol needs l + 2 < bits(N) anyway. */
int sc_initiator_step1(sc_ctx* ctx, int paillier_key, int l, const uint32_t* x_enc_dptr, const uint32_t* y_enc_dptr,
                       const uint32_t* r_dptr, const uint32_t* rho_z_dptr /* nullable */, int flags, uint32_t* z_out_dptr, uint64_t* alpha_dptr,
                       uint64_t* alpha_tilde_dptr, uint64_t* rsmall_dptr, uint32_t* rshift_dptr, uint64_t count);
/* KeyHolder.step_2 + step_4a + step_4b (+ the l + 1 .randomize() of SC/keyholder.py:106-108 when r_rand is given): decrypt z,
 * derive beta / d / zeta_1 / zeta_2, and encrypt d and the bits of beta bit-major: d_beta_out[l+1][count][nwords(n)], plane 0 =
 * [d], plane 1 + i = [beta_i].  z_out: [count][nwords(N)]; beta: flag rows [count][ceil(l/64)] uint64; dbit uint64. */
int sc_keyholder_step2_4b(sc_ctx* ctx, int paillier_key, int dgk_key, int l, const uint32_t* z_enc_dptr,
                          const uint32_t* r_rand_dptr /* nullable */, int r_words, int flags, uint32_t* z_out_dptr, uint64_t* beta_dptr,
                          uint64_t* dbit_dptr, uint32_t* zeta1_dptr, uint32_t* zeta2_dptr, uint32_t* d_beta_out_dptr, uint64_t count);
/* Initiator.step_4c .. step_4i for a batch (SC/initiator.py:272-516): one inversion pass over [d], [beta_i], the fused steps
 * 4c-4h (sc_dgk_step4), then -- when rhos is given -- the blinding c_i^rho_i (:512), the re-randomization * h^r_i when r_rand is
 * given (:153-154) and the shuffle when permutation ([count][l+1] int64, output k takes blinded c at index permutation[b][k]) is
 * given (:516; a row that is not a permutation of 0 .. l acts as the identity), the last three in ONE launch whose store
 * is the shuffle (each item finds its output plane in the permutation row itself: no destination array, no extra launch).  beta: [l][count][nwords] bit-major; rhos / r_rand:
 * [l+1][count][words].  c_unblinded_out (nullable) receives the output of step 4h.  c_out: [l+1][count][nwords].
 * FLAG WORDS (here and in sc_initiator_step67): rsmall and delta_a hold 0 or 1 per comparison and only BIT 0 is read -- alpha and
 * alpha_tilde are flag rows of bit fields (bit i = the i-th bit of r mod 2^l, of (r - N) mod 2^l; [count][ceil(l/64)] uint64), so
 * every flag of a step is taken by position;
 * a caller's own "true" must be the integer 1 (sc_initiator_step1 and sc_rng_coins produce exactly that). */
int sc_initiator_step4(sc_ctx* ctx, int dgk_key, int l, const uint32_t* d_enc_dptr, const uint32_t* beta_enc_dptr,
                       const uint64_t* alpha_dptr, const uint64_t* alpha_tilde_dptr, const uint64_t* rsmall_dptr,
                       const uint64_t* delta_a_dptr, const uint32_t* rhos_dptr /* nullable */, int rho_words,
                       const int64_t* permutation_dptr /* nullable */, const uint32_t* r_rand_dptr /* nullable */, int r_words, int flags,
                       uint32_t* c_unblinded_out_dptr /* nullable */, uint32_t* c_out_dptr, uint64_t count);
/* Step 4i on its own (blinding, optional re-randomization, optional shuffle) for a vector c_in[l+1][count][nwords] that is already
 * there (SC/initiator.py:487-516, :153-154); c_out must not be c_in when a permutation is given. */
int sc_initiator_step4i(sc_ctx* ctx, int dgk_key, int l, const uint32_t* c_in_dptr, const uint32_t* rhos_dptr, int rho_words,
                        const int64_t* permutation_dptr /* nullable */, const uint32_t* r_rand_dptr /* nullable */, int r_words, int flags,
                        uint32_t* c_out_dptr, uint64_t count);
/* KeyHolder.step_4j + step_5 (+ the 3 .randomize() of SC/keyholder.py:126-128 when rho3 is given): delta_B per comparison,
 * then out3[3][count][2 nwords] = [[zeta_1]], [[zeta_2]], [[delta_B]]; rho3: [3][count][nwords] in the same order. */
int sc_keyholder_step4j_5(sc_ctx* ctx, int paillier_key, int dgk_key, int l, const uint32_t* c_enc_dptr, const uint32_t* zeta1_dptr,
                          const uint32_t* zeta2_dptr, const uint32_t* rho3_dptr /* nullable */, int flags, uint64_t* delta_b_out_dptr,
                          uint32_t* out3_dptr, uint64_t count);
/* Initiator.step_6 + step_7 (SC/initiator.py:518-564) with one inversion pass: out = [[x <= y]], not randomized. */
int sc_initiator_step67(sc_ctx* ctx, int paillier_key, const uint64_t* delta_a_dptr, const uint32_t* delta_b_enc_dptr,
                        const uint32_t* zeta1_enc_dptr, const uint32_t* zeta2_enc_dptr, const uint64_t* rsmall_dptr,
                        const uint32_t* rshift_dptr, int flags, uint32_t* out_dptr, uint64_t count);

/* ---- secure selection and compare-exchange: what selection.py / sorting.py do per step, one call each ------ */
/* After a comparison [[delta]] = [[x <= y]] one more round trip selects between encrypted columns: for a selector [[sigma]], sigma in
 * {0, 1}, and columns j < nfields with bases [[b_j]] and differences [[d_j]], d_j = a_j - b_j + 2^w_j, the result is
 * [[b_j + sigma (a_j - b_j)]].  A minimum is (five comparison calls,) select_d, one_minus, select_pack | keyholder_select_mult |
 * select_finish; a compare-exchange of a sort is select_d, cx_differences, select_pack | keyholder_select_mult | cx_finish
 * ("Selection and sort from C").  LAYOUT: (kappa, nfields, widths_hptr) as sc_select_prep takes it -- 1 <= kappa <= 62
 * statistical blinding bits, 1 <= nfields <= 4 columns, widths_hptr[j] = w_j >= 1 (column 0 is the compared value: w_0 = l).  Every
 * entry checks it against the key before anything is launched (SC_ERR_ARG, sc_last_error names the column): the packed fields
 * s + sum_j (w_j + kappa + 2), s = kappa + 1, and every product of s + w_j + kappa + 2 bits must stay below bits(N) - 1.  All
 * ciphertext arrays are [..][count][2 nwords] modulo N^2.  Scratch comes from the context; the work runs on its stream.  Every
 * Paillier key of sc_paillier_key_create is served: where the modulus has no pair kernel with per-row exponents the entries compose
 * the same residues from exponentiations modulo N^2 themselves (no SC_ERR_UNSUPPORTED for that reason). */
/* Initiator.  [[d]] = [[y - x + 2^l]] = [[z]] (1 - r N) from step 1's z_out and its draw r [count][nwords]: no inversion. */
int sc_initiator_select_d(sc_ctx* ctx, int paillier_key, const uint32_t* z_enc_dptr, const uint32_t* r_dptr, uint32_t* d_out_dptr,
                          uint64_t count);
/* [[1 - c]] = (N + 1) [[c]]^-1: the selector of a minimum from [[x <= y]] (8b).  One batched inversion: synchronous like
 * sc_initiator_step67; SC_ERR_NOT_INVERTIBLE names the element through sc_last_bad_index.  out must not overlap c. */
int sc_paillier_one_minus(sc_ctx* ctx, int paillier_key, const uint32_t* c_dptr, uint32_t* out_dptr, uint64_t count);
/* Initiator, compare-exchange (8c): [[d_j]] = [[G_j]] [[F_j]]^-1 (1 + 2^w_j N) for the columns j >= 1; column 0 of d_out is a copy of
 * d_key (the comparison's own [[d]], sc_initiator_select_d).  f_enc / g_enc / d_out: [nfields][count][2 nwords].  One inversion pass
 * over the columns j >= 1 (synchronous, SC_ERR_NOT_INVERTIBLE as above, the index counts from column 1), then one launch for all
 * of them.  nfields = 1: the copy alone. */
int sc_initiator_cx_differences(sc_ctx* ctx, int paillier_key, int kappa, int nfields, const int* widths_hptr, const uint32_t* f_enc_dptr,
                                const uint32_t* g_enc_dptr, const uint32_t* d_key_dptr, uint32_t* d_out_dptr, uint64_t count);
/* Initiator, the message P = [[sigma]] prod_j [[d_j]]^(2^off_j) (1 + R N) rho_p^N with R = r_a + sum_j 2^off_j r_b_j, and the two
 * plaintext arrays the finish needs: e_out[j] = r_b_j + 2^w_j [nfields][count][ew] and rab_out[j] = r_a r_b_j [nfields][count][nwords]
 * (sc_select_prep's outputs).  r_a: [count][aw], aw <= 2, below 2^kappa; r_b: [nfields][count][bw], column j below 2^(w_j + 1 + kappa);
 * 32 ew >= max_j (w_j + kappa + 2); rho_p: [count][nwords] in [1, N).  rho_p is NOT nullable (SC_ERR_ARG): without a fresh rho_p^N
 * the key holder could recognise the ciphertexts he sent earlier inside P. */
int sc_initiator_select_pack(sc_ctx* ctx, int paillier_key, int kappa, int nfields, const int* widths_hptr, const uint32_t* sigma_enc_dptr,
                             const uint32_t* d_enc_dptr, const uint32_t* r_a_dptr, int aw, const uint32_t* r_b_dptr, int bw,
                             const uint32_t* rho_p_dptr, int ew, uint32_t* p_out_dptr, uint32_t* e_out_dptr, uint32_t* rab_out_dptr,
                             uint64_t count);
/* Key holder (secret key): CRT decryption of P, the field products a b_j (sc_select_split), their encryptions randomized with
 * rho_products [nfields][count][nwords]: out [nfields][count][2 nwords].  SC_ERR_LAYOUT when a decrypted row has a bit at or above the
 * end of the announced layout (the initiator packed a WIDER one; `out` is unspecified then).  A narrower one cannot be seen in P:
 * compare the two players' (kappa, widths) on the wire as well.  Synchronous (the verdict is read before it returns). */
int sc_keyholder_select_mult(sc_ctx* ctx, int paillier_key, int kappa, int nfields, const int* widths_hptr, const uint32_t* p_enc_dptr,
                             const uint32_t* rho_products_dptr, uint32_t* out_dptr, uint64_t count);
/* Initiator: out[j] = [[b_j + sigma (a_j - b_j)]] = [[b_j]] [[a b_j]] T_j^-1 with T_j = [[sigma]]^(e_j) [[d_j]]^(r_a) (1 + rab_j N),
 * [nfields][count][2 nwords]; products = the key holder's answer, e / rab = sc_initiator_select_pack's.  One inversion (synchronous,
 * SC_ERR_NOT_INVERTIBLE as above, flat index j count + i), then one launch. */
int sc_initiator_select_finish(sc_ctx* ctx, int paillier_key, int kappa, int nfields, const int* widths_hptr, const uint32_t* sigma_enc_dptr,
                               const uint32_t* d_enc_dptr, const uint32_t* b_enc_dptr, const uint32_t* products_dptr,
                               const uint32_t* r_a_dptr, int aw, const uint32_t* e_dptr, int ew, const uint32_t* rab_dptr,
                               uint32_t* out_dptr, uint64_t count);
/* Initiator, both outputs of a compare-exchange (8c) from the selection with sigma = delta, base F and d = G - F + 2^w: T as above,
 * U = T [[a b]], one inversion of U, then sc_select_finish_cx's launch: lo = G T^2 U^-1, hi = F ab^2 U^-1.  lo_index / hi_index
 * (both or neither): uint64 [nfields][count], the row of out [out_rows][2 nwords] each output goes to; rows >= out_rows are not
 * written.  Both null: out is [2][nfields][count][2 nwords] = (lo, hi) and out_rows >= 2 nfields count. */
int sc_initiator_cx_finish(sc_ctx* ctx, int paillier_key, int kappa, int nfields, const int* widths_hptr, const uint32_t* delta_enc_dptr,
                           const uint32_t* d_enc_dptr, const uint32_t* f_enc_dptr, const uint32_t* g_enc_dptr, const uint32_t* products_dptr,
                           const uint32_t* r_a_dptr, int aw, const uint32_t* e_dptr, int ew, const uint32_t* rab_dptr,
                           const uint64_t* lo_index_dptr /* nullable */, const uint64_t* hi_index_dptr /* nullable */, uint32_t* out_dptr,
                           uint64_t out_rows, uint64_t count);
/* ---- secure multiplication: [[x y_j]] from [[x]] and up to four columns [[y_j]], one round trip ------------------ */
/* The one operation Paillier lacks, with both factors blinded: the initiator packs A = x + e_y and B_j = y_j + e_x_j into one message,
 * the key holder returns fresh [[A B_j]], and [[x y_j]] = [[A B_j]] T_j^-1 with T_j = [[x]]^(e_x_j) [[y_j]]^(e_y) (1 + e_x_j e_y N).
 * LAYOUT: (kappa, wx, nfields, wy_hptr): 1 <= kappa <= 62 statistical blinding bits, 1 <= nfields <= 4 columns, widths 1 .. 255 with
 * 0 <= x < 2^wx, 0 <= y_j < 2^wy[j], or -2^(w-1) <= value < 2^(w-1) as residues modulo N when is_signed.  s = wx + kappa + 1,
 * fbits_j = wy[j] + kappa + 1; every entry checks s + sum_j fbits_j < bits(N) - 1 and every s + fbits_j < bits(N) - 1 against the key
 * before anything is launched (SC_ERR_ARG, sc_last_error names the column).  Arrays, scratch, stream and the keys served: as the
 * selection entries above (no SC_ERR_UNSUPPORTED where the modulus has no pair kernel with per-row exponents).
 * Initiator, the message P = [[x]] prod_j [[y_j]]^(2^off_j) (1 + R N) rho_p^N and the plaintext arrays the finish needs: e_out
 * [nfields + 1][count][ew] (e_x_j = r_b_j + oy_j per column, the LAST plane e_y = r_a + ox; the offsets are 2^(w-1) when is_signed,
 * else 0) and rab_out[j] = e_x_j e_y [nfields][count][nwords].  y_enc: [nfields][count][2 nwords]; r_a: [count][aw] below
 * 2^(wx + kappa); r_b: [nfields][count][bw], column j below 2^(wy[j] + kappa); aw, bw <= 10; 32 ew >= max(s, max_j fbits_j); rho_p:
 * [count][nwords] in [1, N).  rho_p is NOT nullable (SC_ERR_ARG), for sc_initiator_select_pack's reason. */
int sc_initiator_mul_pack(sc_ctx* ctx, int paillier_key, int kappa, int wx, int nfields, const int* wy_hptr, int is_signed,
                          const uint32_t* x_enc_dptr, const uint32_t* y_enc_dptr, const uint32_t* r_a_dptr, int aw,
                          const uint32_t* r_b_dptr, int bw, const uint32_t* rho_p_dptr, int ew, uint32_t* p_out_dptr,
                          uint32_t* e_out_dptr, uint32_t* rab_out_dptr, uint64_t count);
/* Key holder (secret key): CRT decryption of P, the field products A B_j (sc_mul_split), their encryptions randomized with
 * rho_products [nfields][count][nwords]: out [nfields][count][2 nwords].  SC_ERR_LAYOUT and synchronous exactly as
 * sc_keyholder_select_mult: a WIDER layout of the initiator is seen in P, a narrower one only on the wire. */
int sc_keyholder_mul(sc_ctx* ctx, int paillier_key, int kappa, int wx, int nfields, const int* wy_hptr, const uint32_t* p_enc_dptr,
                     const uint32_t* rho_products_dptr, uint32_t* out_dptr, uint64_t count);
/* Initiator: out[j] = base[j] [[x y_j]]^coef, [nfields][count][2 nwords], coef in {+1, -1, -2}; base (nullable: no factor) has the
 * shape of out.  products = the key holder's answer, e / rab = sc_initiator_mul_pack's.  coef = +1 inverts T_j, a negative coef
 * inverts [[A B_j]] and multiplies T_j [[A B_j]]^-1 (squared for -2): one inversion pass either way (synchronous,
 * SC_ERR_NOT_INVERTIBLE names the flat index j count + i through sc_last_bad_index), then one launch.  With base = [[a]] [[b]] on
 * encrypted bits, coef = -1 is a OR b = a + b - a b and coef = -2 is a XOR b = a + b - 2 a b. */
int sc_initiator_mul_finish(sc_ctx* ctx, int paillier_key, int kappa, int wx, int nfields, const int* wy_hptr, const uint32_t* x_enc_dptr,
                            const uint32_t* y_enc_dptr, const uint32_t* products_dptr, const uint32_t* e_dptr, int ew,
                            const uint32_t* rab_dptr, const uint32_t* base_dptr /* nullable */, int coef, uint32_t* out_dptr,
                            uint64_t count);
/* ---- secure inner product: [[sum_j x_j y_j]] from k pairs per row, one round trip, one ciphertext back ------------ */
/* The multiplication's round trip with the sum taken by the key holder under the blinding: the initiator packs the blinded pairs
 * (A_j, B_j) = (x_j + a_j, y_j + b_j), g to a message and M = ceil(k / g) messages per row, the key holder returns ONE fresh [[D]],
 * D = sum_j A_j B_j, and [[sum_j x_j y_j]] = [[D]] T^-1 with T = prod_j [[x_j]]^(b_j) [[y_j]]^(a_j) (1 + S N), S = sum_j a_j b_j.
 * square != 0 computes [[sum_j x_j^2]]: no y, no b, D = sum_j A_j^2, T = prod_j [[x_j]]^(2 a_j) (1 + S N), S = sum_j a_j^2.
 * LAYOUT (kappa, wx, wy, is_signed, square, k): one width per side, 1 <= wx, wy <= 255 (wy is not read for a square), 1 <= kappa <= 62,
 * 1 <= k <= 1024; 0 <= x_j < 2^wx, 0 <= y_j < 2^wy, or -2^(w-1) <= value < 2^(w-1) as residues modulo N when is_signed.  sa = wx +
 * kappa + 1, sb = wy + kappa + 1 (0 for a square), pb = sa + sb; g = the largest integer with g pb < bits(N) - 1 must be >= 1, and
 * pb' + ceil(log2 k) < bits(N) - 1 with pb' = sa + sb (2 sa for a square) keeps the sum below N; M = ceil(k / g); pair j lives in
 * message j mod M at position j div M; ebits = max(sa, sb), sa + 1 for a square.  sc_dot_layout evaluates that rule on the host alone
 * (no context, no device work): out = {sa, sb, pb, g, M, ebits}, SC_ERR_ARG when a quantity is out of range or does not fit.  Every
 * entry below checks the same rule against its key before anything is launched (SC_ERR_ARG, sc_last_error names the quantity).
 * Arrays, scratch, stream and the keys served: as the multiplication's entries (no SC_ERR_UNSUPPORTED where the modulus has no pair
 * kernel with per-row exponents).  Still SC_ABI_VERSION 5: additions. */
int sc_dot_layout(int nbits_n, int kappa, int wx, int wy, int is_signed, int square, int k, int* out /* sa, sb, pb, g, M, ebits */);
/* Initiator, the messages P_m = prod_t [[x_(tM+m)]]^(2^(t pb)) [[y_(tM+m)]]^(2^(t pb + sa)) (1 + R_m N) rho_p_m^N and the plaintext
 * arrays the finish needs.  x_enc, y_enc: [k][count][2 nwords]; r_a: [k][count][aw] below 2^(wx + kappa), r_b: [k][count][bw] below
 * 2^(wy + kappa), aw, bw <= 10 -- an independent mask per field: the key holder sees every A_j of a row, a shared mask would show
 * him x_i - x_j; rho_p: [M][count][nwords] in [1, N), NOT nullable (SC_ERR_ARG), for sc_initiator_select_pack's reason.  p_out:
 * [M][count][2 nwords]; e_out: [2k][count][ew] (planes 0 .. k-1 = b_j, k .. 2k-1 = a_j; for a square [k][count][ew] = 2 a_j),
 * 32 ew >= ebits; s_out: [count][nwords] = S.  y_enc and r_b are not read for a square (null allowed). */
int sc_initiator_dot_pack(sc_ctx* ctx, int paillier_key, int kappa, int wx, int wy, int is_signed, int square, int k,
                          const uint32_t* x_enc_dptr, const uint32_t* y_enc_dptr, const uint32_t* r_a_dptr, int aw,
                          const uint32_t* r_b_dptr, int bw, const uint32_t* rho_p_dptr, int ew, uint32_t* p_out_dptr,
                          uint32_t* e_out_dptr, uint32_t* s_out_dptr, uint64_t count);
/* Key holder (secret key): CRT decryption of the M count messages, D = sum_j A_j B_j per row (sc_dot_split), its encryption randomized
 * with rho_d [count][nwords]: out [count][2 nwords], one ciphertext per row whatever k is.  SC_ERR_LAYOUT when a decrypted message
 * has a bit at or above its own end (`out` is unspecified then); a narrower layout is seen only on the wire.  Synchronous. */
int sc_keyholder_dot(sc_ctx* ctx, int paillier_key, int kappa, int wx, int wy, int square, int k, const uint32_t* p_enc_dptr,
                     const uint32_t* rho_d_dptr, uint32_t* out_dptr, uint64_t count);
/* Initiator: out = base [[sum_j x_j y_j]]^coef, [count][2 nwords], coef in {+1, -1, -2} and base (nullable) as
 * sc_initiator_mul_finish's.  d_enc = the key holder's answer, e / s = sc_initiator_dot_pack's.  T is built from per-row
 * exponentiations over groups of at most three consecutive planes, then ONE inversion pass over count items (synchronous,
 * SC_ERR_NOT_INVERTIBLE names the row through sc_last_bad_index) and one launch. */
int sc_initiator_dot_finish(sc_ctx* ctx, int paillier_key, int kappa, int wx, int wy, int square, int k, const uint32_t* x_enc_dptr,
                            const uint32_t* y_enc_dptr, const uint32_t* d_enc_dptr, const uint32_t* e_dptr, int ew,
                            const uint32_t* s_dptr, const uint32_t* base_dptr /* nullable */, int coef, uint32_t* out_dptr,
                            uint64_t count);
/* ---- secure one-hot encoding and table lookup by an encrypted index: blind, decrypt, rotate -------------------------- */
/* From [[i]] the k ciphertexts [[ [t == i mod k] ]], t < k, in one round trip; sc_initiator_dot_pack / sc_keyholder_dot /
 * sc_initiator_dot_finish over these planes (width 1) and a table's planes then give [[table[i]]] in a second one.  Per row and index
 * q < m the initiator draws r_q < 2^(ib + kappa) and sends the field d_q = i_q + r_q, f = ib + kappa + 1 bits, g fields to a message at
 * the bit offsets 0, f, 2f, .. and M = ceil(m / g) messages per row: index q lives in message q div g at position q mod g, so only the
 * last message may hold fewer than g fields.  The key holder decrypts, takes j_q = d_q mod k and returns E[q][t] = [[ [t == j_q] ]],
 * every one freshly randomized; the initiator reads out[q][t] = E[q][(t + r_q mod k) mod k], a gather of rows.
 * PRECONDITION 0 <= i_q < 2^ib.  The result marks position i_q mod k: an index at or above k is reduced, not refused.
 * LAYOUT (kappa, ib, k, m): 1 <= kappa <= 62, 1 <= ib <= 32, 1 <= k <= 1024, 1 <= m <= 65536 and the one fit rule f < bits(N) - 1; then
 * g = floor((bits(N) - 2) / f).  sc_onehot_layout evaluates that rule on the host alone (no context, no device work): out = {f, g, M, rw}
 * with rw = ceil((ib + kappa) / 32) the words of a mask; SC_ERR_ARG when a quantity is out of range or does not fit.  Every entry below
 * checks the same rule against its key, then its arrays in the order of its parameters, before anything is launched (SC_ERR_ARG,
 * sc_last_error names the argument).  m k count < 2^31.  Arrays, scratch, stream and the keys served: as the inner product's entries.
 * Still SC_ABI_VERSION 5: additions. */
int sc_onehot_layout(int nbits_n, int kappa, int ib, int k, int m, int* out /* f, g, M, rw */);
/* Initiator, the messages P_mm = prod_j [[i_(mm g + j)]]^(2^(j f)) (1 + R_mm N) rho_p_mm^N with R_mm = sum_j 2^(j f) r_(mm g + j), and the
 * rotations the finish needs.  index_enc: [m][count][2 nwords]; r: [m][count][rw] below 2^(ib + kappa), rw <= 3 and 32 rw >= ib + kappa --
 * an independent mask per index; rho_p: [M][count][nwords] in [1, N), NOT nullable (SC_ERR_ARG), for sc_initiator_select_pack's reason.
 * p_out: [M][count][2 nwords]; rot_out: [m][count] int32 = r mod k, taken over all the words of r. */
int sc_initiator_onehot_pack(sc_ctx* ctx, int paillier_key, int kappa, int ib, int k, int m, const uint32_t* index_enc_dptr,
                             const uint32_t* r_dptr, int rw, const uint32_t* rho_p_dptr, uint32_t* p_out_dptr, int32_t* rot_out_dptr,
                             uint64_t count);
/* Key holder (secret key): CRT decryption of the M count messages, the m k count plaintexts [t == d_q mod k] (sc_onehot_split), their
 * encryptions randomized with rho_e [m][k][count][nwords]: e_out [m][k][count][2 nwords].  SC_ERR_LAYOUT when a decrypted message has a
 * bit at or above its own end (`e_out` is unspecified then); a narrower layout is seen only on the wire.  Synchronous. */
int sc_keyholder_onehot(sc_ctx* ctx, int paillier_key, int kappa, int ib, int k, int m, const uint32_t* p_enc_dptr,
                        const uint32_t* rho_e_dptr, uint32_t* e_out_dptr, uint64_t count);
/* Initiator: out[q][t][b] = e_enc[q][(t + rot[q][b]) mod k][b], both [m][k][count][2 nwords]; rot = sc_initiator_onehot_pack's.  One
 * launch, no arithmetic modulo N^2.  out must not overlap e_enc (SC_ERR_ARG). */
int sc_initiator_onehot_finish(sc_ctx* ctx, int paillier_key, int kappa, int ib, int k, int m, const uint32_t* e_enc_dptr,
                               const int32_t* rot_dptr, uint32_t* out_dptr, uint64_t count);
/* The network of a secure top-m (8d): the comparators that bring the m smallest of k values to the positions 0 .. m-1 in ascending
 * order -- with only_last, the m-th smallest to position m-1 alone -- for 1 <= m <= k <= 1024 (SC_ERR_ARG otherwise).  Host only: no
 * context, no device work, a pure function of (k, m, only_last) that both players evaluate.  Comparator t puts the smaller value at
 * ij_out[t][0] < ij_out[t][1]; keep_out[t][0 / 1] is 1 when that output is read again (by a later comparator or as a result) and 0 when
 * it is dead: hand sc_initiator_cx_finish the index out_rows for a dead output and it is not written.  Comparators come layer by
 * layer, the comparators of a layer are disjoint, and layer_end_out[t] is the number of comparators in the layers 0 .. t.  The three
 * arrays hold `cap` entries; cap >= *n_comparators >= *n_layers is enough.  cap = 0 (the arrays may be null) only reports the sizes;
 * a cap in between reports them and returns SC_ERR_ARG.  m = k without only_last is the full sort's network, every flag 1.  Still
 * SC_ABI_VERSION 5: an addition. */
int sc_topk_network(int k, int m, int only_last, int cap, int32_t* ij_out /* [cap][2] */, uint8_t* keep_out /* [cap][2] */,
                    int32_t* layer_end_out /* [cap] */, int* n_comparators, int* n_layers);

/* ---- secure division by public divisors: [[x div d]] and [[x mod d]], exact floor division ---------------------------- */
/* [[x]] with 0 <= x < 2^x_bits and a public divisor 1 <= d < 2^64 per row.  The comparison is this division with d = 2^l, so the calls
 * a host already has carry it: the initiator blinds, z = x + r with r < 2^(x_bits + kappa) (sc_initiator_div_blind, which also returns
 * rq = r div d and rm = r mod d); the key holder decrypts and divides (sc_keyholder_div_open: zq = z div d, zm = z mod d); then both run
 * the DGK sub-comparison [[zm < rm]] at l = max(1, bits(max d - 1)) through sc_dgk_encrypt_bits_randomized (the bit 1, then the l bits
 * of zm), sc_initiator_step4 (alpha = alpha_tilde = rm, r_small = 1), sc_keyholder_step4j_5 (zeta_1 = zeta_2 = zq) and
 * sc_initiator_step67 (r_small = 1, r_shift = rq), whose result is [[zq]] ([[rq]] [[zm < rm]])^-1 = [[x div d]].  The DGK key needs
 * u > 2^(l + 2).  INTEGRATION.md section 2b has the sequence.
 * The fit rule, 1 when it holds and 0 when not: x_bits + kappa + 2 < nbits_n - 1 with 1 <= kappa <= 62 and x_bits >= 1, so that z never
 * wraps around N and stays below (N - 1) / 2.  is_signed: -2^x_bits <= x < 2^x_bits; the caller divides x + c d, c = ceil(2^x_bits / d),
 * and subtracts c from the quotient, and the rule holds for the offset dividend's width max(x_bits + 2, 65) in place of x_bits.  Host
 * only, no context. */
int sc_div_fits(int nbits_n, int kappa, int x_bits, int is_signed);
/* Initiator: z_out [count][2 nwords] = [[x + r]] rho^N from x_enc [count][2 nwords] (signed input: the offset [[x + c d]]), r
 * [count][nwords] (< 2^(x_bits + kappa), zero-extended to the words of N) and rho [count][nwords] -- or, with SC_STEP_RANDOMIZERS_READY
 * in flags, the finished randomizers rho^N [count][2 nwords]; rq_out [count][nwords] = r div d and rm_out [count] uint64 = r mod d for
 * the divisors d [count] uint64 (device).  SC_ERR_ARG before anything is launched where sc_div_fits refuses.
 * ZERO DIVISORS: the call queues its launches and cannot see a divisor of zero.  A host that has not checked d itself MUST call
 * sc_ctx_synchronize(ctx) after this call (and after sc_keyholder_div_open) and before it uses rq, rm (zq, zm): that is the one place
 * where the error comes back -- SC_ERR_ARG, once, the affected rows written as zero -- and a host that never synchronises through the
 * context never sees it, while a later, unrelated sc_ctx_synchronize would (sc_plain_divmod, sc_amd_dev.h). */
int sc_initiator_div_blind(sc_ctx* ctx, int paillier_key, int kappa, int x_bits, int is_signed, const uint32_t* x_enc_dptr,
                           const uint32_t* r_dptr, const uint32_t* rho_dptr, int flags, const uint64_t* d_dptr, uint32_t* z_out_dptr,
                           uint32_t* rq_out_dptr, uint64_t* rm_out_dptr, uint64_t count);
/* Key holder: z = Dec([[z]]) for z_enc [count][2 nwords], then zq_out [count][nwords] = z div d and zm_out [count] uint64 = z mod d.
 * The decryption, then one division launch in place; a zero divisor as above. */
int sc_keyholder_div_open(sc_ctx* ctx, int paillier_key, const uint32_t* z_enc_dptr, const uint64_t* d_dptr, uint32_t* zq_out_dptr,
                          uint64_t* zm_out_dptr, uint64_t count);

/* ---- device-side CSPRNG: the random draws of a batch, generated where they are consumed ---------------- */
/* The reference draws from Python's `secrets` (SC/initiator.py:223 permutation, :250 r, :420 delta_A, :512 rho_i) and the
 * scheme packages draw the randomizers behind every .randomize() ([ext]).  A batch of 65536 comparisons needs ~0.3 GB of such
 * draws per step; these entry points produce them on the device from a counter-mode generator: the ChaCha20 block function
 * (RFC 8439 2.3), keystream(call, item) = ChaCha20_block(key, counter = 0, 1, .., nonce = (item, call_lo, call_hi)) read as
 * little-endian words, `call` = number of generator calls on this context since it was seeded.  Asynchronous on the stream.
 *   sc_rng_seed:         32-byte key from the OS (NULL: getrandom) or from the caller -- the latter for TESTS and known-answer
 *                        vectors only: seeding resets the call counter, so the same key replays the same streams.  An unseeded
 *                        context seeds itself from the OS on first use.  A context belongs to one host thread at a time (see the
 *                        conventions above); the call counter is atomic all the same, so two threads that did share a context
 *                        would never draw one (key, call) pair twice.
 *   sc_rng_bits:         out[count][ceil(bits/32)]: uniform below 2^bits (DGK randomizer exponents).
 *   sc_rng_below:        out[count][nwords]: uniform in [0, n) or, nonzero != 0, in [1, n), by rejection sampling on the device
 *                        (r below N, rho_i in [1, u), Paillier randomizer bases in [1, N)); n must fill its top word.
 *   sc_rng_coins:        out[count] uint64, each 0 or 1 (delta_A).
 *   sc_rng_permutations: out[count][k] int64: one uniform permutation of 0 .. k-1 per item (Fisher-Yates with rejection-sampled
 *                        indices; the step-4i shuffle, handed to sc_initiator_step4 / _step4i as `permutation`). */
int sc_rng_seed(sc_ctx* ctx, const uint8_t* key32_hptr /* nullable */);
int sc_rng_bits(sc_ctx* ctx, int bits, uint32_t* out_dptr, uint64_t count);
int sc_rng_below(sc_ctx* ctx, const uint32_t* n_hptr, int nwords, int nonzero, uint32_t* out_dptr, uint64_t count);
int sc_rng_coins(sc_ctx* ctx, uint64_t* out_dptr, uint64_t count);
int sc_rng_permutations(sc_ctx* ctx, int k, int64_t* out_dptr, uint64_t count);

/* ---- multi-GPU ---------------------------------------------------------------------- */
/* The comparisons of a batch are independent: every rank (one process and one context per GPU) runs all steps on its own block
 * with no traffic during compute; the only exchange is the reassembly of the ranks' result blocks -- [[x <= y]], or the per-bit
 * vectors in the blocked layout [rank][l+1][B/ranks][words] -- by ONE all-gather (RCCL over xGMI) on the context's stream.  The
 * reference has no counterpart (its only concurrency is session_id namespacing, SC/initiator.py:86-87).  RCCL is loaded on first
 * use (dlopen), so single-GPU users never need it.
 *   sc_comm_unique_id: rank 0 creates the 128-byte rendezvous id (SC_COMM_ID_BYTES); the caller ships it to the other ranks.
 *   sc_comm_init:      every rank joins with the same id (collective call).
 *   sc_allgather:      recv[r * words_per_rank ..] = rank r's send[0 .. words_per_rank) for every r; asynchronous on the stream.
 *   sc_comm_destroy:   also done by sc_ctx_destroy. */
#define SC_COMM_ID_BYTES 128
int sc_comm_unique_id(sc_ctx* ctx, void* id_hptr);
int sc_comm_init(sc_ctx* ctx, const void* id_hptr, int rank, int nranks);
int sc_allgather(sc_ctx* ctx, const uint32_t* send_dptr, uint32_t* recv_dptr, uint64_t words_per_rank);
int sc_comm_destroy(sc_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* SC_AMD_H */

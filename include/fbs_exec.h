/*
 * fbs_exec.h -- C ABI of libfbsexec.so, the MI355X (gfx950) executor for the
 * "linear combination + functional bootstrap" programs of ssmiler/tfhe_fbs_map.
 *
 * The reference has NO native/FFI boundary: its executor is the Python method
 * `LutExecEnv.eval` (fbs_mapper/fbs_exec_env.py:208-229) and the only call
 * site is fbs_mapper/map_circuit.py:174.  This header is therefore the
 * boundary a maintainer would bind with ctypes from that method (stub in
 * INTEGRATION.md).  Each entry point names the reference construct it stands
 * behind.
 *
 * Conventions: every function returns 0 on success and a negative FBS_E_* code
 * on failure (never throws, never aborts: every entry point is an exception
 * barrier -- a host allocation that fails inside the library comes back as
 * FBS_E_NOMEM, any other internal exception as FBS_E_INVALID -- and counts are
 * checked against FBS_MAX_* before anything is sized by them; what the library
 * cannot check is that a caller's array is as long as its count says);
 * `fbs_last_error` gives the text.
 * Host buffers are caller-allocated, C-contiguous, 64-bit words unless stated;
 * the library owns device memory and keys behind opaque handles.  A context is
 * bound to one GPU and must be driven by one host thread at a time.  There is
 * no CPU fallback: without a usable gfx950 device `fbs_ctx_create` fails.
 *
 * Ciphertexts are LWE samples over Z_q, q = 2^46 - 62*2^13 + 1 = 0x3FFFFFF84001
 * (prime; the ciphertext modulus and the NTT modulus are the same), one residue
 * per 64-bit word, under the "big" key of dimension D = k*N: D mask words then
 * the body, all canonical (< q).  A message m in [0, 2p) is encoded as
 * m * Delta, Delta = 2*round(q/4p), with p = `p_msg` the reference's `fbs_size`
 * (map_circuit.py:97,117-122).
 *
 * Streams.  Entry points that take a `stream` queue their work on it and return
 * without waiting -- except a call that needs more scratch than any earlier one,
 * which blocks while the scratch grows (fbs_ctx_reserve sizes it up front).  All
 * calls on a context share its scratch buffers: calls on one stream are ordered
 * by the stream, and a call on a different stream first waits (on the device)
 * for the previous call that used the scratch.
 */
#ifndef FBS_EXEC_H
#define FBS_EXEC_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FBS_OK 0
#define FBS_E_INVALID (-1)   /* bad argument / unsupported parameter set          */
#define FBS_E_DEVICE (-2)    /* HIP error (no GPU, OOM, launch failure ...)       */
#define FBS_E_STATE (-3)     /* call out of order (e.g. eval before keygen)       */
#define FBS_E_TABLE (-4)     /* table violates the negacyclic contract for p      */
#define FBS_E_POLY_SIZE (-5) /* polynomial size rejected (see fbs_poly_size_check) */
#define FBS_E_NOMEM (-6)     /* the HOST could not allocate what the arguments ask for */

typedef struct fbs_params {
    uint32_t n;          /* small LWE dimension (P1024: 630)                      */
    uint32_t log_n_poly; /* log2 of the GLWE polynomial size N (P1024: 10)        */
    uint32_t k;          /* GLWE dimension: 1 (N = 256 .. 4096); 2, 3, 4 at N = 256 / 512; 2, 3 at N = 1024 (any l_bsk, bsk_group 1 or 2) */
    uint32_t l_bsk;      /* blind-rotation gadget levels (3)                      */
    uint32_t beta_bsk;   /* log2 blind-rotation gadget base (7)                   */
    uint32_t t_ksk;      /* key-switch levels (8)                                 */
    uint32_t gamma_ksk;  /* log2 key-switch base (2)                              */
    uint32_t p_msg;      /* plaintext modulus p = fbs_size                        */
    uint64_t sigma_lwe;  /* std-dev of key-switch-key noise, in units of 1/q       */
    uint64_t sigma_glwe; /* std-dev of bootstrap-key and fresh-input noise, same  */
    uint32_t bsk_group;  /* key bits consumed per blind-rotation step: 0 or 1 = one   */
                         /* (n CMUX steps); 2 = two ("multi-bit": n/2 steps on a     */
                         /* bundle of three GGSW samples per pair of key bits; n even)*/
    union {              /* noise sampler of every key and fresh encryption (RANDOMNESS GRADE below):   */
        uint32_t sampler;    /* 0 = Irwin-Hall(12), reproducible / test-grade, the default; 1 = rounded     */
                             /* Gaussian; anything else is refused (FBS_E_INVALID)                          */
        uint32_t reserved;   /* the field's name before it had a meaning: sources that set it to 0 compile  */
    };
} fbs_params;

/* Polynomial sizes.  fbs_params carries log2 N: the ring is Z_q[X]/(X^N + 1) with N a power of two (this build:
 * 256 .. 4096).  BASELINE config 5 also names "non-power-of-two N".  That is rejected on purpose, not for lack of a
 * transform (2N | q - 1 holds for N = 3 * 2^k under this modulus): for N = m * 2^k with m odd > 1, X^N + 1 is not
 * cyclotomic -- y^m + 1 is divisible by y + 1, so X^N + 1 has the factor X^(2^k) + 1 and every GLWE sample maps onto
 * the power-of-two ring of degree N/m, whose (smaller) dimension then bounds the security: N = 1536 is no safer than
 * N = 512 and costs three times as much.  The reference's patch generalises the plaintext modulus p, not N
 * (experiments/concrete.patch:85-90); odd p at power-of-two N is what this library runs for that config.
 * Returns FBS_OK, FBS_E_POLY_SIZE for a non-power-of-two (text via fbs_last_error(NULL)), FBS_E_INVALID for a power
 * of two outside the supported range. */
int fbs_poly_size_check(uint32_t poly_size);

typedef struct fbs_ctx fbs_ctx;
typedef struct fbs_tvset fbs_tvset;
typedef struct fbs_prog fbs_prog;

/* ---- context ------------------------------------------------------------ */
/* device: HIP ordinal.  seed: all key material and encryption randomness is
 * derived from it (ChaCha20 streams, DESIGN.md "Randomness").
 *
 * RANDOMNESS GRADE.  fbs_ctx_create is the REPRODUCIBLE form: 64 bits of seed, the
 * same keys for the same seed whatever the parameter set -- for tests, benchmarks
 * and checkers that must be keyed identically (oracle/).  It is not a way to make
 * production keys, whatever noise the parameter set carries.  fbs_ctx_create_seeded
 * keys the generator with 32 caller-supplied bytes (e.g. from the OS) and mixes the
 * parameter set into the derivation, so that two parameter sets under one seed
 * share no key material.
 *
 * The noise of every key row and every fresh encryption comes from the sampler
 * fbs_params.sampler names, in BOTH forms, on the host and on the device alike:
 *   0  an integer Irwin-Hall(12) stand-in for a discrete Gaussian: a sum of twelve
 *      uniform 32-bit terms, bounded at 6 sigma, excess kurtosis -0.1.  Reproducible,
 *      test-grade, and the DEFAULT: the oracle and the committed known-answer tests
 *      pin its streams word for word.  Making 1 the default is a later decision.
 *   1  a rounded Gaussian: Box-Muller in double precision (the library's own ln, sin
 *      and cos, bit-identical on host and device, z to better than 2^-46 relative)
 *      on 128 + 53 bits of the ChaCha20 stream keyed from the caller's seed -- with
 *      fbs_ctx_create_seeded, the caller's 32 bytes -- scaled by sigma and rounded to
 *      the nearest integer, ties to even.  Its tail reaches sqrt(2 128 ln 2) = 13.3
 *      sigma.  It is NOT constant-time (it branches on its random words), NOT a
 *      certified discrete Gaussian (a continuous Gaussian evaluated in doubles and
 *      rounded; no bound on its statistical or Renyi distance from one is claimed),
 *      and it has NOT been audited.  sigma is accepted up to q.
 * A sampler-1 context under fbs_ctx_create_seeded shares no key material with its
 * sampler-0 twin (the sampler is mixed into the derivation when it is not 0).  A
 * deployment that needs more than either brings its own keys with fbs_import_keys. */
#define FBS_DEVICE_NONE (-1)   /* `device` of a context of the client library (below); libfbsexec.so refuses it like any ordinal it has no GPU for */
int fbs_ctx_create(const fbs_params *params, uint64_t seed, int device, fbs_ctx **out);
int fbs_ctx_create_seeded(const fbs_params *params, const uint8_t seed[32], int device, fbs_ctx **out);
void fbs_ctx_destroy(fbs_ctx *ctx);
/* Scratch (modulus-switched rows, the key switch's digit/limb buffers, accumulators of shared rotations, the wire
 * buffer of fbs_eval) grows on demand, and growing BLOCKS: the call that needs more than any earlier one waits for
 * the context's queued work, frees and reallocates.  A host that wants every *_dev call to be kernel launches and
 * nothing else (several streams, collectives between levels) sizes it once: max_keyswitches = the largest number
 * of key switches one call will ask for (fbs_bootstrap_batch_dev: count; fbs_level_bootstrap_dev: the slice's
 * sources x samples; fbs_eval_dev: fbs_layout.max_sources x T), max_shared_rows = shared rotations x samples of a
 * fused program's widest level (0 otherwise), wire_words = n_slots x T x (D+1) for fbs_eval_dev (0 otherwise).
 * Zero leaves a buffer as it is.  After it, the only blocking case left is a call that exceeds what was reserved. */
int fbs_ctx_reserve(fbs_ctx *ctx, size_t max_keyswitches, size_t max_shared_rows, size_t wire_words);
/* Launcher knobs -- which kernel shape a launch takes.  The defaults are the measured choices; tests set them to reach
 * every kernel instantiation at small sizes.  Results never depend on them.
 *   "ks_mfma" (1)           0: no int8 GEMM on the matrix cores for the key switch
 *   "ks_fp" (1)             0: ... and the integer kernels instead of the FP64 one
 *   "br_cu_kernel" (1)      launches of up to two bootstraps per CU as ONE bootstrap per CU (eight or twelve waves)
 *   "br_cu_lean" (1)        ... and between one and two per CU as two 128-register workgroups per CU (2: always, 0: never)
 *   "br_k2_shape" (0)       GLWE dimension 2: 0 by launch size, 3 always three waves per bootstrap, 12 always twelve
 *   "br_glwe_fpw" (0)       other GLWE dimensions >= 2: bootstraps per workgroup, 0 by launch size; 1, 2; larger: the
 *                           throughput shape
 *   "pack_slices" (0)       packed outputs: slices the i-sum of one packed sample is cut into, 0 by launch size (at most 32)
 *   "keys_on_device" (0)    1: fbs_keygen, fbs_keygen_seeded, fbs_import_seeded_keys and fbs_packing_keygen make (expand) the
 *                           evaluation keys on the GPU instead of on host threads ("keys", below); every key word is the same */
int fbs_ctx_tune(fbs_ctx *ctx, const char *knob, int64_t value);
/* counters: "scratch_growths" (how often a call (re)allocated scratch, i.e. blocked), "ms_capacity", "acc_capacity",
 * "wires_capacity", "next_nonce", "cu_count"; "has_secret" (1: the context holds secret keys), "seeded_keys" (1: its keys
 * came from fbs_keygen_seeded or fbs_import_seeded_keys); "states_alive", "state_bytes" (resident state: fbs_state blocks not
 * yet destroyed, and the device bytes they hold); "packing_key" (1: the context holds a packing key), "packing_levels" and
 * "packing_base_bits" (its t_p and gamma_p, 0 without one); "fold_key", "fold_levels" and "fold_base_bits" (the same for the fold
 * key of "folded state": t_f and gamma_f); "keys_made_on_device" (1: the keys held now were made or expanded
 * on the GPU, knob "keys_on_device"), "bsk_upload_bytes" (bytes of bootstrapping-key material the last key-making call copied
 * host -> device: the whole key on the host path, 0 for keys made on the device, the bodies for a server key expanded there) */
int fbs_ctx_stat(const fbs_ctx *ctx, const char *name, int64_t *value);
/* text of the last failure on `ctx` (or of the last failed fbs_ctx_create when ctx == NULL) */
const char *fbs_last_error(const fbs_ctx *ctx);
/* "gfx950 <device name> CUs=<n>" of the bound device */
const char *fbs_device_info(const fbs_ctx *ctx);

/* ---- keys ----------------------------------------------------------------
 * Secret keys stay on the host; the bootstrapping key (n GGSW samples) is
 * uploaded, transformed to the NTT domain on the GPU and kept resident, as is
 * the key-switching key.  The GLWE secret key (the big key ciphertexts are
 * encrypted under) also lives in device memory, as packed bits, for the life
 * of the context: the device encryption and decryption below read it.
 *
 * Knob "keys_on_device" = 1 (fbs_ctx_tune; default 0) moves the making of both
 * evaluation keys to the GPU: the secrets are still drawn on the host and are
 * uploaded first, the key rows are made from the same ChaCha20 streams, the same
 * sampler and an exact negacyclic product by the secret, and the bootstrapping
 * key is transformed from the device rows -- it is not uploaded at all.  The
 * rows are copied back as the host copies that fbs_export_keys and
 * fbs_export_seeded_keys read and that the key-switching tables are derived
 * from (on the host, either way).  Every key word is what the host path makes:
 * results never depend on the knob.  It covers fbs_keygen, fbs_keygen_seeded,
 * fbs_import_seeded_keys (only the bodies are uploaded; the masks are expanded
 * on the GPU) and the bodies of fbs_packing_keygen; fbs_import_keys takes full
 * keys from the caller and is not affected. */
int fbs_keygen(fbs_ctx *ctx);
/* word counts of { sk_lwe, sk_glwe, bsk, ksk } in the standard (coefficient) layout:
 *   sk_lwe[n], sk_glwe[k][N] (bit c N + j = coefficient j of key polynomial S_c; read flat it is the key of the
 *     extracted LWE ciphertexts, dimension k N);
 *   bsk[G][(k+1) l][k+1][N]: GGSW sample g, row rr = comp l + lv (comp = 0 .. k: the GLWE component the gadget
 *     factor sits on, k = the body; lv = gadget level), then the row's k + 1 polynomials: columns 0 .. k-1 the mask
 *     A_0 .. A_(k-1), column k the body B = sum_c A_c S_c + e -- and the message: bit g_lv added to coefficient 0
 *     of column comp, g_lv = round(q / 2^(beta (lv+1)));
 *     bsk_group <= 1: G = n, sample g encrypts key bit sk_lwe[g];
 *     bsk_group = 2 (the default 128-bit sets): G = 3 n / 2, samples 3 i, 3 i + 1, 3 i + 2 belong to the pair
 *     (s0, s1) = (sk_lwe[2 i], sk_lwe[2 i + 1]) and encrypt s0 (1 - s1), (1 - s0) s1 and s0 s1, in that order;
 *   ksk[k N][t][n+1]: row (j, v) = LWE under sk_lwe (n mask words, then the body) of sk_glwe[j] h_v,
 *     h_v = round(q / 2^(gamma (v+1))), j = c N + coefficient. */
int fbs_key_sizes(const fbs_ctx *ctx, size_t sizes[4]);
/* test hook: copy keys out (any pointer may be NULL) so a checker can be keyed identically */
int fbs_export_keys(const fbs_ctx *ctx, uint64_t *sk_lwe, uint64_t *sk_glwe, uint64_t *bsk, uint64_t *ksk);
/* The mirror: keys made elsewhere (a caller's own CSPRNG and Gaussian sampler, or a checker's) in the layout of
 * fbs_key_sizes, instead of fbs_keygen.  Secret keys are binary, every other word a canonical residue (< q); the
 * evaluation keys must encrypt the secrets under this library's gadget conventions (GGSW row
 * (c, l) = GLWE(0) + s g_l on component c, g_l = round(q / 2^(beta (l+1))); key-switching row (j, v) = LWE(s_j h_v)).
 * The secret keys stay on the host and serve fbs_encrypt / fbs_decrypt only.  Besides the ranges, the call DECRYPTS a few
 * GGSW samples (first, middle, last; every row) and key-switching rows with the supplied secrets and refuses
 * (FBS_E_INVALID) keys whose phases are not what this layout says they encrypt, within 16 standard deviations of the
 * parameter set's noises: a key in another order fails here, not as garbage after the first bootstrap. */
int fbs_import_keys(fbs_ctx *ctx, const uint64_t *sk_lwe, const uint64_t *sk_glwe, const uint64_t *bsk, const uint64_t *ksk);

/* ---- encrypt / decrypt (host side, big key) ------------------------------
 * Stand behind the Input arm of eval (fbs_exec_env.py:213-214) and the final
 * read-out (:225-229).  Ciphertext i draws its randomness from stream
 * nonce0 + i, so a run is reproducible. cts: [count][D+1]. */
int fbs_encrypt(const fbs_ctx *ctx, const int64_t *msgs, size_t count, uint64_t nonce0, uint64_t *cts);
/* The same on streams nobody has used: the context keeps a counter over [2^55, 2^56) (fbs_encrypt's explicit nonces stay
 * below 2^55), so two calls never share mask or noise.  *nonce0 (may be NULL) = the first stream this call took. */
int fbs_encrypt_fresh(fbs_ctx *ctx, const int64_t *msgs, size_t count, uint64_t *cts, uint64_t *nonce0);
/* msgs[i] = round(phase * 2p / q) mod 2p */
int fbs_decrypt(const fbs_ctx *ctx, const uint64_t *cts, size_t count, int64_t *msgs);
/* The same three on device buffers, asynchronous on `stream` (NULL = the context's own stream), word-identical to
 * fbs_encrypt / fbs_encrypt_fresh / fbs_decrypt: the same streams, checks, error codes and nonce rules (a refused call writes
 * nothing and leaves the stream counter where it was; count = 0 does nothing).  d_msgs [count] int64, d_cts [count][D+1].
 * They use no per-context scratch. */
int fbs_encrypt_dev(const fbs_ctx *ctx, const int64_t *d_msgs, size_t count, uint64_t nonce0, uint64_t *d_cts, void *stream);
int fbs_encrypt_fresh_dev(fbs_ctx *ctx, const int64_t *d_msgs, size_t count, uint64_t *d_cts, uint64_t *nonce0, void *stream);
int fbs_decrypt_dev(const fbs_ctx *ctx, const uint64_t *d_cts, size_t count, int64_t *d_msgs, void *stream);

/* ---- seeded keys and inputs: evaluation without the secret key --------------
 * A client holds the secret; a server evaluates with the evaluation keys only.  Every mask of this path is drawn from
 * ChaCha20 under a PUBLIC 32-byte mask key (the first 32 bytes of a ChaCha20 block under the context's key, which that
 * block does not reveal), so a server regenerates the masks and only bodies travel: a bootstrapping-key row shrinks from
 * (k+1) N words to N, a key-switching row from n + 1 words to one, an input ciphertext from D + 1 words to one.  Noise and secrets
 * come from the context's key, on streams of their own: no noise stream is shared with fbs_keygen
 * or fbs_encrypt.  The secrets are drawn as fbs_keygen draws them, so a client may mix seeded and full calls.
 *
 * fbs_keygen_seeded: as fbs_keygen, with the seeded streams.  The keys it uploads are full keys in the layout of
 * fbs_key_sizes (fbs_export_keys reads them); a mask row of a GGSW sample carries its message in the body
 * (-bit g_lv S_comp), which is the phase -- and the distribution -- of fbs_keygen's rows. */
int fbs_keygen_seeded(fbs_ctx *ctx);
/* word counts of the bodies: sizes[0] = G (k+1) l N (bsk_bodies[G][(k+1) l][N], column k of every bootstrapping-key
 * row), sizes[1] = k N t (ksk_bodies[k N][t], word n of every key-switching row) */
int fbs_seeded_key_sizes(const fbs_ctx *ctx, size_t sizes[2]);
/* the server key: mask key and bodies.  FBS_E_STATE unless the keys came from fbs_keygen_seeded on this context. */
int fbs_export_seeded_keys(const fbs_ctx *ctx, uint8_t mask_key[32], uint64_t *bsk_bodies, uint64_t *ksk_bodies);
/* The mirror, on the server: expands (mask key, bodies) into full keys on the host and uploads them (knob "keys_on_device":
 * uploads the bodies and expands them on the GPU; the same checks, codes and texts, the same keys).  Every body word must
 * be a canonical residue (FBS_E_INVALID otherwise).  The phases cannot be checked, because there is no secret: keys
 * made for another parameter set or mask key are accepted and bootstrap to garbage.  A refused call leaves the previous
 * keys in place and usable.  Afterwards the context is EVALUATION-ONLY: its secret keys are gone from host and device,
 * and every entry that needs them (fbs_encrypt*, fbs_decrypt*, fbs_eval_messages, fbs_encrypt_seeded*,
 * fbs_export_seeded_keys, fbs_export_keys with sk_lwe or sk_glwe non-NULL) returns FBS_E_STATE; everything else works
 * as after fbs_keygen.  fbs_keygen / fbs_import_keys / fbs_keygen_seeded make it a full context again. */
int fbs_import_seeded_keys(fbs_ctx *ctx, const uint8_t mask_key[32], const uint64_t *bsk_bodies, const uint64_t *ksk_bodies);
/* Seeded encryption: bodies[count] only.  Ciphertext i takes stream nonce0 + i (mask and noise), under fbs_encrypt's nonce
 * rules: explicit nonces below 2^55, fresh ones from the counter fbs_encrypt_fresh uses. */
int fbs_encrypt_seeded(const fbs_ctx *ctx, const int64_t *msgs, size_t count, uint64_t nonce0, uint64_t *bodies);
int fbs_encrypt_seeded_fresh(fbs_ctx *ctx, const int64_t *msgs, size_t count, uint64_t *bodies, uint64_t *nonce0);
/* the same two on device buffers, asynchronous on `stream` (NULL = the context's own), word-identical to the host entries */
int fbs_encrypt_seeded_dev(const fbs_ctx *ctx, const int64_t *d_msgs, size_t count, uint64_t nonce0, uint64_t *d_bodies,
                           void *stream);
int fbs_encrypt_seeded_fresh_dev(fbs_ctx *ctx, const int64_t *d_msgs, size_t count, uint64_t *d_bodies, uint64_t *nonce0,
                                 void *stream);
/* bodies[count] of streams nonce0 .. nonce0 + count - 1 (below 2^56) -> full ciphertexts cts [count][D+1] under the
 * context's mask key; needs no secret.  fbs_expand_seeded runs on the host and is the reference the device entry is held to. */
int fbs_expand_seeded(const fbs_ctx *ctx, const uint64_t *bodies, size_t count, uint64_t nonce0, uint64_t *cts);
int fbs_expand_seeded_dev(const fbs_ctx *ctx, const uint64_t *d_bodies, size_t count, uint64_t nonce0, uint64_t *d_cts,
                          void *stream);

/* ---- client library: libfbsclient.so, the secret-key holder's part of this header on a machine with no GPU ------------------------
 * The party that makes the keys, encrypts the inputs and reads the results is not the party with the GPU.  libfbsclient.so is
 * built from the host sources alone (make -C tfhe_fbs_map_amd/csrc client: a C++17 compiler, no ROCm, no HIP runtime among its
 * dependencies) and exports a SUBSET of the entries declared here, with the signatures, checks, error codes and nonce rules
 * given above -- the two libraries compile the same code for them:
 *     poly_size_check, ctx_create, ctx_create_seeded, ctx_destroy, ctx_stat, last_error, device_info,
 *     keygen, key_sizes, export_keys,   keygen_seeded, seeded_key_sizes, export_seeded_keys,
 *     encrypt, encrypt_fresh, decrypt,   encrypt_seeded, encrypt_seeded_fresh, expand_seeded,
 *     compact_words, decrypt_compact,   packing_keygen, packing_key_sizes, export_packing_key, packed_words, decrypt_packed,
 *     debug_raise                                                                      (each with the fbs_ prefix).
 * Every other entry is ABSENT from that library, not stubbed: a program that needs one links libfbsexec.so.  Every entry is an
 * exception barrier, as there.
 * THE CONTRACT.  For the same fbs_params and the same seed, in either seed form, every word the client library writes -- secret
 * keys, full keys, the mask key, key bodies, packing-key bodies, ciphertexts, seeded bodies, the streams fresh calls take -- is the
 * word libfbsexec.so writes, and every message it decodes is the message libfbsexec.so decodes.  A server key exported by one opens
 * in the other.
 * DIFFERENCES from libfbsexec.so:
 *   - `device` must be FBS_DEVICE_NONE.  Any other value returns FBS_E_DEVICE, with a text that names libfbsexec.so as the library
 *     for contexts on a GPU.  The sentence at the top of this header stays true of libfbsexec.so: it has no CPU fallback, and
 *     FBS_DEVICE_NONE does not give it one.
 *   - the device-info entry returns "host".
 *   - the statistics served are "has_secret", "seeded_keys", "next_nonce", "packing_key", "packing_levels" and "packing_base_bits";
 *     any other name returns FBS_E_INVALID.
 *   - parameter admission is the same: the range rules, then whether libfbsexec.so has kernels for the set (a set it refuses is
 *     refused here with the same code, since no server could evaluate under such keys).
 *   - a context is host memory only, so nothing is uploaded: the packing keygen entry keeps the bodies, the export entries read them. */

/* ---- tables -> test vectors ----------------------------------------------
 * One entry per distinct `Bootstrap.table` (fbs_exec_env.py:51-61).  Table t is
 * table_vals[table_off[t] .. table_off[t+1]); length <= 2p, and where it
 * exceeds p it must satisfy table[i] + table[i+p] == const (the three modes of
 * map_to_fbs.py:81-98), else FBS_E_TABLE. */
int fbs_tvset_create(fbs_ctx *ctx, const int32_t *table_vals, const uint32_t *table_off, uint32_t n_tables,
                     fbs_tvset **out);
void fbs_tvset_destroy(fbs_tvset *tv);

/* ---- batch of independent functional bootstraps (BASELINE config 2) -------
 * One FBS = key switch (kN -> n), modulus switch (q -> 2N), blind rotation
 * (n CMUX), sample extraction: the encrypted form of `table[v]`
 * (fbs_exec_env.py:218-220).  Host buffers: cts_in/out [count][D+1]. */
int fbs_bootstrap_batch(fbs_ctx *ctx, const fbs_tvset *tv, const uint64_t *cts_in, const uint32_t *table_ids,
                        size_t count, uint64_t *cts_out);
/* same on device-resident buffers, asynchronous on `stream` (a hipStream_t; NULL = the
 * context's own stream).  d_table_ids is a device array of `count` uint32; being device
 * memory it cannot be checked by the host: an id >= the set's size selects table 0. */
int fbs_bootstrap_batch_dev(fbs_ctx *ctx, const fbs_tvset *tv, const uint64_t *d_cts_in,
                            const uint32_t *d_table_ids, size_t count, uint64_t *d_cts_out, void *stream);

/* ---- linear combination (LinearProd, fbs_exec_env.py:37-49, :215-217) ------
 * out[g][s] = sum_i coefs[off[g]+i] * wires[srcs[off[g]+i]][s] + consts[g]*Delta  for g < n_out,
 * s < T.  `d_wires` is a device array laid out [wire][T][D+1]; outputs are written to wire
 * slots dst[g] of the same array.  term_off has n_out+1 entries.  HOST index arrays: this call
 * and fbs_bootstrap_wires_dev stage them through a per-context buffer and wait for that copy
 * (a convenience for tests and one-off calls; to step a program use fbs_level_* below). */
int fbs_lincomb_dev(fbs_ctx *ctx, uint64_t *d_wires, size_t T, uint32_t n_out, const uint32_t *dst,
                    const uint32_t *term_off, const uint32_t *srcs, const int64_t *coefs, const int64_t *consts,
                    void *stream);
/* bootstraps over wire slots: wire dst[g] = FBS(wire src[g], table table_ids[g]) for samples
 * [s_begin, s_end) of each gate (the slice a rank owns in gate-sharded multi-GPU mode). */
int fbs_bootstrap_wires_dev(fbs_ctx *ctx, const fbs_tvset *tv, uint64_t *d_wires, size_t T, uint32_t n_gates,
                            const uint32_t *src, const uint32_t *dst, const uint32_t *table_ids, size_t s_begin,
                            size_t s_end, void *stream);

/* ---- whole program (LutExecEnv.eval, fbs_exec_env.py:208-229) ---------------
 * Flat description of `LutExecEnv.instructions` after the Input entries:
 *   wire ids: 0..n_inputs-1 are the inputs in program order, n_inputs+i is
 *   instruction i.  kind[i]: 0 = LinearProd, 1 = Bootstrap.
 *   LinearProd i: terms [arg0[i], arg0[i]+arg1[i]) of (term_coef, term_src), constant const_coef[i].
 *   Bootstrap  i: source wire arg0[i], table id arg1[i] (into the fbs_tvset).
 *   outputs: out_wire[o] >= 0 is a wire id; a constant output c is encoded as -1-c. */
#define FBS_MAX_WIRES (1u << 28)   /* n_inputs + n_instr, and n_outputs, of one program */
#define FBS_MAX_TERMS (1u << 30)   /* n_terms of one program */
#define FBS_MAX_TABLES (1u << 20)  /* tables of one fbs_tvset */
typedef struct fbs_program_desc {
    uint32_t n_inputs, n_instr, n_terms, n_outputs;
    const uint8_t *kind;
    const uint32_t *arg0, *arg1;
    const int64_t *const_coef;
    const int64_t *term_coef;
    const uint32_t *term_src;
    const int64_t *out_wire;
} fbs_program_desc;

int fbs_program_load(fbs_ctx *ctx, const fbs_program_desc *desc, const fbs_tvset *tv, fbs_prog **out);
/* The same with options.  FBS_LOAD_FUSE_TABLES: several tables on ONE blind rotation (the reference's
 * one-gate-one-bootstrap lowering puts several tables on one linear combination, fbs_mapper/map_to_fbs.py:41-45, and its
 * CSE merges identical tables only, fbs_exec_env.py:93-100).  A source wire that two or more Bootstraps read is rotated
 * ONCE, from the table-independent test vector TV_0 = Delta/2 (1 + X + .. + X^(N-1)); each table F is then cut out of that
 * accumulator by a product with the small integer polynomial D_F (TV_F = TV_0 * D_F; multi-value bootstrap, Carpov,
 * Izabachene, Mollimard, CT-RSA 2019) and a sample extraction.  Same decrypted results; such an output carries more noise
 * than an ordinary bootstrap's (fbs_table_fusion_norms: the caller's parameter choice must carry it), and the ciphertexts
 * differ from the unfused program's.  Into the wire slots a level of a fused program runs whole (fbs_eval, fbs_eval_dev,
 * fbs_level_bootstrap_dev over the full range without d_rows).  Across GPUs the unit dealt out is the ROTATION:
 * fbs_level_bootstrap_dev with d_rows takes any slice of the level's (rotation, sample) grid, its rows are
 * fbs_layout.row_words = (k + 1) N words -- an ordinary gate leaves its ciphertext there, a shared rotation its whole accumulator --
 * and fbs_level_scatter_dev, given all rows of the level, files the ciphertexts and cuts every table out of the gathered
 * accumulators. */
#define FBS_LOAD_FUSE_TABLES 1u
int fbs_program_load_ex(fbs_ctx *ctx, const fbs_program_desc *desc, const fbs_tvset *tv, uint32_t flags, fbs_prog **out);
/* What sharing a rotation does to the noise of table `table`'s output, with TV_F = Delta/2 G_F(X) (G_j = +-(2 f - c)):
 * *d_norm2 = |D_F|^2, *g_norm2 = |G_F|^2 (sums over the N coefficients).  The part of the blind-rotation noise that comes
 * from the bootstrapping key's noise has independent coefficients and grows by |D_F|^2; the part that comes from rounding
 * the accumulator is seen through the BINARY key S, whose mean 1/2 makes S D_F = G_F / 2 + (centred part) D_F: it grows
 * by |D_F|^2 / 2 + |G_F|^2 / (2N).  max of the two bounds the variance factor for any mix. */
int fbs_table_fusion_norms(const fbs_tvset *tv, uint32_t table, uint64_t *d_norm2, uint64_t *g_norm2);
void fbs_program_destroy(fbs_prog *prog);
/* depth (number of bootstrap levels) and the widest level, as scheduled */
int fbs_program_info(const fbs_prog *prog, uint32_t *n_levels, uint32_t *max_width, uint32_t *n_bootstrap);
/* in_cts: host [n_inputs][T][D+1]; out_cts: host [n_outputs][T][D+1] (constant outputs are
 * written as trivial ciphertexts).  Levels are batched over (gate, sample); samples are
 * evaluated in chunks whose wire slots fit in HBM. */
int fbs_eval(fbs_ctx *ctx, fbs_prog *prog, const uint64_t *in_cts, size_t T, uint64_t *out_cts);
/* the same on device-resident buffers, asynchronous on `stream` */
int fbs_eval_dev(fbs_ctx *ctx, fbs_prog *prog, const uint64_t *d_in, size_t T, uint64_t *d_out, void *stream);
/* Messages in, messages out: fbs_eval with the inputs encrypted on the device straight into their wire slots and the output
 * slots decrypted there, so only int64 messages cross the bus.  msgs: host [n_inputs][T]; out_msgs: host [n_outputs][T].
 * Input i, sample s takes stream nonce0 + i*T + s (the order fbs_encrypt gives a [n_inputs][T] array).  fresh != 0:
 * n_inputs*T streams are reserved from the context's counter (as fbs_encrypt_fresh) and the first is written to *nonce0
 * (may be NULL); fresh == 0: *nonce0 is read, under fbs_encrypt's range rule.  The results are those of fbs_decrypt applied
 * to fbs_eval of fbs_encrypt's ciphertexts; a constant output reads back as fbs_decrypt of the trivial ciphertext fbs_eval
 * returns for it.  T = 0 does nothing.  Blocks until the messages are back. */
int fbs_eval_messages(fbs_ctx *ctx, fbs_prog *prog, const int64_t *msgs, size_t T, int fresh, uint64_t *nonce0,
                      int64_t *out_msgs);
/* Seeded inputs, full outputs: bodies host [n_inputs][T] (fbs_encrypt_seeded of a [n_inputs][T] array: input i, sample s
 * on stream nonce0 + i*T + s), out_cts host [n_outputs][T][D+1] as fbs_eval returns them (constant outputs as trivial
 * ciphertexts).  Only the bodies cross the bus on the way in; they are expanded on the device straight into the input
 * wire slots.  The same chunks as fbs_eval; needs no secret.  T = 0 does nothing.  Blocks until the outputs are back. */
int fbs_eval_seeded(fbs_ctx *ctx, fbs_prog *prog, const uint64_t *bodies, size_t T, uint64_t nonce0, uint64_t *out_cts);

/* ---- compact outputs: what a server returns in place of big-key ciphertexts ----------------------------------------------
 * A compact ciphertext at width `bits` = w, log2(2N) <= w <= 31, is the big-key ciphertext key-switched to the small LWE key
 * (dimension n) with the key-switching key, which gives x in Z_q^(n+1) (mask first, body last), then rounded to Z_(2^w) exactly
 * as the modulus switch rounds to Z_2N before every blind rotation, with q treated as 2^46:
 *     sh = 46 - w;   m_i = ((x_i >> (sh-1)) + 1) >> 1  (i < n);   eps = sum_i (x_i - (m_i << sh))  (signed);
 *     body' = (x_n - floor(eps / 2)) mod q;   m_n = ((body' >> (sh-1)) + 1) >> 1;   every field mod 2^w.
 * At w = log2(2N) the fields are, word for word, what the blind rotation reads.  PACKING: a ciphertext is
 * W = ceil((n+1) w / 64) uint64 words; field j occupies bits [j w, j w + w) of the ciphertext's bit stream, stream bit b being
 * bit b mod 64 of word b / 64; bits past the last field are zero; a batch is [count][W].  DECODE under the small key s:
 *     phase = (m_n - sum_i m_i s_i) mod 2^w;   msg = ((phase 2p + 2^(w-1)) >> w) mod 2p.
 * The compaction of a constant output is that of its trivial ciphertext: zero mask fields and the rounded body.  The noise it
 * carries is at most that of a bootstrap input at w = log2(2N) (params.compact_output_variance).
 * Every entry returns FBS_E_INVALID for a w outside [log2(2N), 31] and writes nothing when it fails. */
int fbs_compact_words(const fbs_ctx *ctx, uint32_t bits, size_t *words);
/* d_cts [count][D+1] (any big-key ciphertexts, device) -> d_words [count][W], asynchronous on `stream`; needs no secret.  Runs in
 * passes of the context's modulus-switch scratch (of at least 8192 ciphertexts): it does not grow scratch with count. */
int fbs_compact_dev(fbs_ctx *ctx, const uint64_t *d_cts, size_t count, uint32_t bits, uint64_t *d_words, void *stream);
/* fbs_eval_seeded with compact outputs: out_words host [n_outputs][T][W], and only those words cross the bus on the way back.
 * Equal to fbs_compact_dev of fbs_eval_seeded's outputs (constant outputs as above).  Needs no secret.  T = 0 does nothing.
 * Blocks until the outputs are back. */
int fbs_eval_seeded_compact(fbs_ctx *ctx, fbs_prog *prog, const uint64_t *bodies, size_t T, uint64_t nonce0, uint32_t bits,
                            uint64_t *out_words);
/* the decode, words [count][W] -> msgs[count]; host and device give the same messages.  FBS_E_STATE on an evaluation-only
 * context (as fbs_decrypt). */
int fbs_decrypt_compact(const fbs_ctx *ctx, const uint64_t *words, size_t count, uint32_t bits, int64_t *msgs);
int fbs_decrypt_compact_dev(const fbs_ctx *ctx, const uint64_t *d_words, size_t count, uint32_t bits, int64_t *d_msgs, void *stream);

/* ---- chained evaluation: one program's outputs as the next one's inputs, under the same evaluation keys ------------------
 * A compact ciphertext goes back into a program through a REFRESH: its fields are unpacked to b = log2(2N) bits into the rows
 * the blind rotation reads -- at w = b word for word what the modulus switch would have left, at w > b re-rounded by the header
 * formula above with 2^w in place of 2^46 (sh = w - b; round the mask fields, eps = sum of their signed errors in 64 bits,
 * body' = (m_n - floor(eps / 2)) mod 2^w, round the body) -- and one blind rotation through the identity table [0, 1, .., p - 1]
 * writes a fresh big-key ciphertext of the same value (every value in [0, p); program inputs are bits).  It costs one bootstrap
 * per ciphertext and carries that bootstrap's noise, whatever the link's.  None of these entries needs a secret.
 *
 * PLAINTEXT INPUTS.  A server brings data of its own (a table row, a round key, a counter) as cleartext messages: a source of kind
 * FBS_SRC_PLAIN holds int64 messages in [0, 2p), the range fbs_encrypt accepts, and the ciphertext of message m is word for word
 * the trivial ciphertext fbs_eval writes for a constant output m: D zero mask words, then m * Delta mod q, Delta = 2*round(q/4p).
 * It is written on the device straight into the input's wire slots: 8 bytes a sample cross the bus, or nothing for a broadcast
 * message.  A trivial ciphertext carries no noise and hides nothing: the messages are public.  The program still pays its
 * bootstraps for such an input; nothing is folded. */
/* d_words [count][W] at width `bits` -> the fields d_fields [count][n + 1] (uint32, < 2^log2(2N)), asynchronous on `stream` */
int fbs_compact_fields_dev(fbs_ctx *ctx, const uint64_t *d_words, size_t count, uint32_t bits, uint32_t *d_fields, void *stream);
/* d_words [count][W] -> refreshed big-key ciphertexts d_cts [count][D+1], asynchronous on `stream`.  At bits = log2(2N) equal
 * to fbs_bootstrap_batch_dev of the ciphertexts fbs_compact_dev packed, through the identity table.  In passes of the
 * modulus-switch scratch (of at least 8192 ciphertexts), like fbs_compact_dev. */
int fbs_refresh_compact_dev(fbs_ctx *ctx, const uint64_t *d_words, size_t count, uint32_t bits, uint64_t *d_cts, void *stream);

#define FBS_SRC_SEEDED 0u    /* the client's seeded inputs: data = [T] bodies of streams nonce0 + s */
#define FBS_SRC_FULL 1u      /* full ciphertexts of an earlier evaluation: data = [T][D+1] */
#define FBS_SRC_COMPACT 2u   /* compact ciphertexts of an earlier evaluation: data = [T][W] at width `bits` */
#define FBS_SRC_PLAIN 3u     /* the server's cleartext messages: data = host int64 [T] (bits = 0) or one message for all T samples (bits = 1) */
typedef struct fbs_input_src {
    uint32_t kind;        /* FBS_SRC_* */
    uint32_t bits;        /* COMPACT: its width w.  PLAIN: 0 = sample s takes data[s], 1 = broadcast, data[0] serves every sample */
    uint32_t refresh;     /* FULL: 1 = bootstrap through the identity table before use (COMPACT: always; SEEDED: never; PLAIN: must be 0) */
    uint64_t nonce0;      /* SEEDED: sample s on stream nonce0 + s (PLAIN: not read) */
    const uint64_t *data; /* host memory (PLAIN: int64 messages behind this pointer) */
} fbs_input_src;
/* One evaluation whose input i comes from src[i], any mix of the four kinds.  out_bits = 0: full outputs out [n_outputs][T][D+1]
 * (as fbs_eval_seeded); else compact outputs out [n_outputs][T][W] at that width (as fbs_eval_seeded_compact).  The same chunks
 * as fbs_eval; full inputs marked `refresh` go through the ordinary key switch and modulus switch, then the identity rotation.
 * With every source seeded at nonce0 + i T the outputs are word for word those of fbs_eval_seeded (out_bits = 0) and of
 * fbs_eval_seeded_compact (out_bits = w).  Refused with FBS_E_INVALID, nothing written: an unknown kind, null data, a compact
 * width outside [log2(2N), 31], streams past 2^56, T * words overflowing, a plaintext message outside [0, 2p) (every message is checked
 * before anything is queued), a plaintext source with refresh != 0 or bits > 1.  Repeated calls of one shape do not grow scratch.
 * T = 0 does nothing.  Blocks until the outputs are back. */
int fbs_eval_sources(fbs_ctx *ctx, fbs_prog *prog, const fbs_input_src *src, size_t T, uint32_t out_bits, uint64_t *out);

/* ---- resident state: chained ciphertexts that stay on the GPU between evaluations ------------------------------------------
 * A server whose state only its own later evaluations read keeps it in device memory: an fbs_state is a context-owned block of
 * big-key ciphertexts laid out [rows][T][D+1].  It is not part of the scratch: it never moves or shrinks while alive, and a
 * growing scratch leaves it alone.  An evaluation writes its outputs into a state (fbs_eval_resident) and a later one reads its
 * inputs from state rows, with no copy to the host and no refresh in between; the state leaves the card only when asked
 * (fbs_state_fetch), full or compact.  Every entry works on the context's own stream, in call order.  None needs a secret. */
typedef struct fbs_state fbs_state;
/* rows, T >= 1; rows <= FBS_MAX_WIRES, and rows * T * (D+1) words must not overflow (FBS_E_INVALID, checked before anything is
 * sized).  A device that cannot hold it: FBS_E_DEVICE, and the context stays usable.  The words are not initialised. */
int fbs_state_create(fbs_ctx *ctx, size_t rows, size_t T, fbs_state **out);
/* Waits for the work queued on the context, then frees.  NULL is allowed.  fbs_ctx_destroy frees the states still alive: a
 * state must not be destroyed after its context. */
void fbs_state_destroy(fbs_state *st);
int fbs_state_info(const fbs_state *st, size_t *rows, size_t *T);   /* (either pointer may be NULL) */

typedef struct fbs_resident_src {
    const fbs_state *state;   /* NULL: input i comes from src[i], as in fbs_eval_sources */
    uint32_t row;             /* input i = row `row` of `state`, all T samples */
    uint32_t refresh;         /* as fbs_input_src.refresh of FBS_SRC_FULL: 1 = key switch, modulus switch and identity rotation first */
} fbs_resident_src;
/* fbs_eval_sources with two additions.  (1) res (may be NULL: no resident input) has one entry per input; where res[i].state is
 * non-NULL input i is that state row and src[i] is not read (src may be NULL when every input is resident).  (2) Exactly one of
 * out_host and out_state is given.  out_host: as `out` of fbs_eval_sources, at out_bits.  out_state (then out_bits must be 0): a
 * state of n_outputs rows whose row o becomes output o for all T samples, a constant output as the trivial ciphertext fbs_eval
 * writes.  The same chunks as fbs_eval: chunk [s0, s0 + tc) reads samples s0 onwards of each state row and writes samples s0
 * onwards of out_state, one gather launch and one scatter launch per chunk.  With out_state and every input resident, seeded
 * or plaintext (FBS_SRC_PLAIN mixes with state rows like the other kinds) the call queues its work on the context's stream and returns without waiting for it (the caller's arrays are read before it
 * returns; a later call on the context, fbs_state_fetch included, is ordered behind it); otherwise it blocks as
 * fbs_eval_sources does.  Refused with FBS_E_INVALID, nothing written: what fbs_eval_sources refuses; a state of another
 * context; a row past the state's rows; a state whose T differs from the call's; an out_state with rows != n_outputs; an
 * out_state that is also an input state (no in-place hops); both or neither of out_host and out_state; out_bits != 0 with
 * out_state.  Repeated calls of one shape do not grow scratch.  T = 0 does nothing. */
int fbs_eval_resident(fbs_ctx *ctx, fbs_prog *prog, const fbs_input_src *src, const fbs_resident_src *res, size_t T, uint32_t out_bits,
                      uint64_t *out_host, fbs_state *out_state);
/* Rows [row0, row0 + rows) to the host.  bits = 0: the full ciphertexts, out [rows][T][D+1].  Else compact words out [rows][T][W]
 * at that width: compacted on the device as fbs_compact_dev does it (word for word fbs_compact_dev of the full fetch), in passes of
 * the modulus-switch scratch, and only the packed words cross the bus.  Blocks until the data is back. */
int fbs_state_fetch(fbs_ctx *ctx, const fbs_state *st, size_t row0, size_t rows, uint32_t bits, uint64_t *out);
/* The way back (state saved to disk by a full fetch): cts [rows][T][D+1] into rows [row0, row0 + rows).  Every word must be a
 * canonical residue (FBS_E_INVALID otherwise, nothing written).  Blocks until the words are on the device. */
int fbs_state_put(fbs_ctx *ctx, fbs_state *st, size_t row0, size_t rows, const uint64_t *cts);

/* ---- sample-axis operations: gather and group sum across the T samples of resident state ------------------------------------
 * Everything above treats the T samples of a call as T independent lanes.  These two entries are the steps ACROSS lanes, on
 * state that stays on the card: an evaluation whose resident inputs read their samples through an index (gather, shift,
 * broadcast, stride, and the pairing of a tree reduction), and the sum of runs of samples (counts and totals).  Neither touches a
 * bootstrap: a gathered ciphertext is the ciphertext it was, and a sum of g ciphertexts carries g times the noise variance, which
 * the consumer removes by refresh = 1.  Neither needs a secret.  Neither is part of the client or public libraries. */
#define FBS_SAMPLE_NONE 0xFFFFFFFFu
typedef struct fbs_sample_map {
    const uint32_t *index;   /* host, [T] entries; NULL: the identity (then the state's T must equal the call's, as today) */
    int64_t fill;            /* message in [0, 2p): sample s with index[s] == FBS_SAMPLE_NONE is its trivial ciphertext */
} fbs_sample_map;
/* fbs_eval_resident with one addition: maps (may be NULL: then this IS fbs_eval_resident, which is a call of this entry) has one
 * entry per input.  Where res[i].state is non-NULL and maps[i].index is non-NULL, sample s of input i is sample index[s] of that
 * state row, whose state may hold any T_src >= 1 samples a row; where index[s] == FBS_SAMPLE_NONE the sample is the trivial
 * ciphertext of `fill`, word for word what FBS_SRC_PLAIN writes for that message.  refresh = 1 works on a mapped input as on any
 * other.  The index arrays are read before the call returns, like the caller's other arrays, and are uploaded once per call;
 * chunk [s0, s0 + tc) reads index[s0 + q].  Unmapped state rows go through the gather launch of fbs_eval_resident; one more
 * launch per chunk moves the mapped ones.  Refused with FBS_E_INVALID, nothing written, besides what fbs_eval_resident refuses:
 * an index entry >= T_src that is not FBS_SAMPLE_NONE; a fill outside [0, 2p); a map (index != NULL) on an input that is not a
 * state row; a NULL index with T_src != T (the rule of fbs_eval_resident).  Every entry is checked before anything is queued.
 * The output state must still not be an input state. */
int fbs_eval_resident_mapped(fbs_ctx *ctx, fbs_prog *prog, const fbs_input_src *src, const fbs_resident_src *res,
                             const fbs_sample_map *maps /* one per input, may be NULL */, size_t T, uint32_t out_bits,
                             uint64_t *out_host, fbs_state *out_state);
/* Sample j of row dst_row0 + r of dst, r < rows, becomes the word-wise sum modulo q of samples [j group, min((j+1) group, T_src))
 * of row row0 + r of src: the ciphertext of the sum of their messages (which the caller keeps inside [0, p)).  Every word of the
 * result is a canonical residue.  dst must hold exactly ceil(T_src / group) samples a row, and src != dst.  1 <= group <=
 * FBS_MAX_SUM_GROUP: 65536 residues below q < 2^46 sum to less than 2^62, so a 64-bit accumulator per word cannot wrap and one
 * reduction at the end gives the residue.  group = 1 is a copy.  Queued on the context's stream like the other state entries (a
 * later fetch or evaluation is ordered behind it).  Refused with FBS_E_INVALID, nothing written: rows past either state's rows; a
 * dst of another T; a state of another context; src == dst; group out of range.  rows = 0 does nothing. */
#define FBS_MAX_SUM_GROUP 65536u
int fbs_state_sum_groups(fbs_ctx *ctx, const fbs_state *src, size_t row0, size_t rows, size_t group,
                         fbs_state *dst, size_t dst_row0);

/* ---- packed outputs: up to N output bits in one GLWE ciphertext under the key the client already holds ------------------------
 * A compact ciphertext costs (n + 1) w bits per output.  A PACKING KEY SWITCH writes up to N of them into the N coefficients of one
 * GLWE sample under the big key (S_0 .. S_(k-1)), (k + 1) N w bits for N outputs.
 *
 * PACKING KEY, parameters (t_p, gamma_p), 1 <= t_p, 1 <= gamma_p, t_p gamma_p <= 31.  (The packing kernel transforms its digits
 * with the general forward transform -- "first=0" in fbs_debug_transform_list, inputs |x| <= q -- so gamma_p has no further bound.)
 * Rows (i, v), i < n, v < t_p, layout [n][t_p][k+1][N]: row (i, v) is a GLWE encryption of the constant polynomial s_i h_v,
 * s = sk_lwe, h_v = round(q / 2^(gamma_p (v+1))): polynomials A_0 .. A_(k-1), then B = sum_c A_c S_c + e + s_i h_v (e: sigma_glwe).
 * The masks come from ChaCha20 under the context's public mask key, the noise from the context's key, both on streams no other
 * key or ciphertext uses ("Randomness"); only the bodies [n][t_p][N] travel.  Every (k, N) a context can be
 * created with is served.  The key belongs to the evaluation keys it was made beside: fbs_keygen, fbs_import_keys,
 * fbs_keygen_seeded and fbs_import_seeded_keys drop it.
 *
 * PACKING.  Input: `count` big-key ciphertexts, in order; ciphertext j goes to coefficient j mod N of sample g = j / N; the last
 * sample may be partly filled (fill f_g <= N).
 *   1. key switch to the small key at width 31, exactly as fbs_compact_dev(bits = 31): fields m_0 .. m_n in Z_(2^31);
 *   2. mask fields to t_p gamma_p bits: r = 31 - t_p gamma_p; r > 0: a' = ((m_i >> (r-1)) + 1) >> 1 mod 2^(t_p gamma_p); r = 0: a' = m_i;
 *   3. a' into t_p BALANCED digits d_v in [-2^(gamma_p - 1), 2^(gamma_p - 1)), v = 0 the most significant: from the least
 *      significant up, u = field + carry; u >= 2^(gamma_p - 1): d = u - 2^gamma_p, carry 1; else d = u, carry 0; the carry out of
 *      the top is dropped (the key switch's own convention);
 *   4. body lifted to Z_q: B_j = (m_n q + 2^30) >> 31, an exact integer;
 *   5. D_(i,v)(X) = sum_j d_v(a' of ciphertext j, field i) X^j;  ACC_c = - sum_(i,v) D_(i,v) A_c^(i,v)  (c < k),
 *      ACC_k = sum_j B_j X^j - sum_(i,v) D_(i,v) B^(i,v);  negacyclic, mod q.
 * Every quantity is an exact residue: the result does not depend on summation order, launch shape or "pack_slices".
 *
 * TRANSPORT.  Width w, log2(2N) <= w <= 31.  Every coefficient x is rounded as the compact format rounds, q treated as 2^46:
 * ((x >> (45 - w)) + 1) >> 1 mod 2^w (no mean compensation).  A sample is its k N mask fields, component-major, then the f_g body
 * fields of coefficients j < f_g; fields of w bits, bit-packed as compact ciphertexts are (stream bit b = bit b mod 64 of word
 * b / 64, zero padding); every sample starts on a word boundary; a batch is its samples back to back: fbs_packed_words.
 * DECODE.  phase_j = body_j - sum_c (A_c S_c)_j mod 2^w;  msg = ((phase 2p + 2^(w-1)) >> w) mod 2p.
 * Noise: params.packed_output_variance.  Every entry returns FBS_E_INVALID for a w outside [log2(2N), 31] and writes nothing when
 * it fails. */
/* Makes the packing key on the host and uploads it in the transform domain.  FBS_E_STATE unless the context's keys came from
 * fbs_keygen_seeded on this context (the masks are the mask key's); FBS_E_INVALID for parameters outside the range above. */
int fbs_packing_keygen(fbs_ctx *ctx, uint32_t t_p, uint32_t gamma_p);
/* word counts for t_p levels (0: the context's own key; FBS_E_STATE without one): sizes[0] = n t_p N (bodies), sizes[1] = n t_p (k+1) N */
int fbs_packing_key_sizes(const fbs_ctx *ctx, uint32_t t_p, size_t sizes[2]);
/* bodies [n][t_p][N] (what a server needs beside the mask key).  full (may be NULL) is a test hook: the whole key
 * [n][t_p][k+1][N] in the coefficient domain, as fbs_export_keys returns the others.  Either pointer may be NULL. */
int fbs_export_packing_key(const fbs_ctx *ctx, uint64_t *bodies, uint64_t *full);
/* The mirror: expands the masks from the context's mask key and uploads.  Works on evaluation-only contexts (after
 * fbs_import_seeded_keys).  Every body word must be a canonical residue (FBS_E_INVALID); a refused call leaves the previous
 * packing key in place. */
int fbs_import_packing_key(fbs_ctx *ctx, uint32_t t_p, uint32_t gamma_p, const uint64_t *bodies);
/* words of a batch of `count` outputs at width `bits`: (count / N) full samples of (k + 1) N w / 64 words, and for a rest
 * f = count mod N > 0 one of k N w / 64 + ceil(f w / 64) */
int fbs_packed_words(const fbs_ctx *ctx, size_t count, uint32_t bits, size_t *words);
/* d_cts [count][D+1] (any big-key ciphertexts, device) -> d_words [fbs_packed_words], asynchronous on `stream`; needs no secret;
 * FBS_E_STATE without a packing key.  Runs in passes of the modulus-switch scratch (whole samples of at least 8192 ciphertexts);
 * its own scratch (the transposed fields of a pass, partial accumulators) grows like any other: repeated calls of one shape do
 * not grow it. */
int fbs_pack_dev(fbs_ctx *ctx, const uint64_t *d_cts, size_t count, uint32_t bits, uint64_t *d_words, void *stream);
/* Rows [row0, row0 + rows) of a resident state, flattened [row][sample] in that order, packed on the device as fbs_pack_dev packs
 * them (word for word fbs_pack_dev of fbs_state_fetch(bits = 0)); only the packed words cross the bus.  Blocks until they are back. */
int fbs_state_fetch_packed(fbs_ctx *ctx, const fbs_state *st, size_t row0, size_t rows, uint32_t bits, uint64_t *out);
/* the decode on the host, words [fbs_packed_words(count)] -> msgs[count].  FBS_E_STATE on an evaluation-only context. */
int fbs_decrypt_packed(const fbs_ctx *ctx, const uint64_t *words, size_t count, uint32_t bits, int64_t *msgs);

/* ---- public-key inputs: encrypt without the secret, expand on the GPU ------------------------------------------------------------
 * A data owner who is neither the key holder nor the server -- a sensor, a second company, a user of a service somebody else
 * keyed -- encrypts under a PUBLIC KEY and sends GLWE samples; the server turns them into big-key ciphertexts by sample
 * extraction, which needs no key at all.  Notation as above: GLWE key S_0 .. S_(k-1) (binary), D = k N, Delta = 2*round(q/4p),
 * negacyclic ring mod q.
 *
 * PUBLIC KEY.  Masks A[r][c], r, c < k: uniform residues under the public mask key (the one the server key carries), on a ChaCha20
 * domain no other key or ciphertext uses: A[r][c]_j = word c N + j of stream (18, r), folded as every other mask is.  Bodies
 * P_r = sum_c A[r][c] S_c + E_r, E_r of standard deviation sigma_glwe from the parameter set's sampler (fbs_params.sampler, both
 * samplers), coefficient j = sample j of stream (19, r) under a 32-byte noise seed the caller passes (the ChaCha20 key itself,
 * little-endian words).  Only the bodies travel, [k][N] words.  The key is k GLWE encryptions of zero under masks the key holder
 * does not choose: as hard as the bootstrapping-key rows, dimension k N at sigma_glwe.  NEVER make two public keys for one secret
 * under one noise seed and different mask keys: their bodies would differ by (A - A') S.
 *
 * ENCRYPTION needs no secret.  GLWE sample g of a call takes stream nu = nonce0 + g under the encryptor's own ChaCha20 key, derived
 * from 32 caller bytes and the parameter set the way fbs_ctx_create_seeded derives a context's:
 *     u_r (r < k) binary: bit j of u_r = bit (r N + j) mod 64 of word (r N + j) / 64 of stream (20, nu);
 *     e_c (c <= k) of standard deviation sigma_glwe: coefficient j = sample c N + j of stream (21, nu);
 *     A'_c = sum_r u_r A[r][c] + e_c  (c < k);     B' = sum_r u_r P_r + e_k + Delta M(X)  mod q.
 * u is a rank-k binary module secret with noise sigma_glwe, exactly as hard to recover as S itself for every (k, N) this library
 * builds -- which is why the key is a k x k matrix and not one ring element (one u in R at k = 3, N = 512 would sit at dimension
 * 512).  The phase is sum_r u_r E_r + e_k - sum_c e_c S_c + Delta M: variance (1 + k N) sigma_glwe^2 (params.public_input_variance),
 * many orders below one blind rotation's output, so a public-key input enters a program unrefreshed.
 * IND-CPA only, and malleable like every ciphertext here: nothing proves that a sample is well formed.  The samplers' caveats
 * (RANDOMNESS GRADE above) apply to E, e and u alike.  Reusing (seed, nonce) reuses u and e: two such samples differ by exactly
 * Delta (M - M') and leak the difference of their messages.
 *
 * WIRE FORMAT.  A sample is [k+1][N] canonical residues in 64-bit words: A'_0 .. A'_(k-1), then B'.  Message j of a call lies at
 * coefficient j mod N of sample j / N (the packed outputs' rule); `count` messages are G = ceil(count / N) samples back to back;
 * coefficients past the fill of the last sample carry message 0 and are never extracted.  Messages lie in [0, 2p).
 *
 * EXPANSION of message j at coefficient t = j mod N into the big-key ciphertext [D+1]:
 *     word c N + i = A'_c[t - i] for i <= t,  (q - A'_c[N + t - i]) mod q for i > t (a zero word stays zero);   word D = B'[t].
 * fbs_decrypt of the result returns the message: the sign convention is the blind rotation's own extraction.
 *
 * RULES.  Parameter sets pass the admission of fbs_ctx_create, with its codes and texts.  Body and sample words must be canonical
 * residues and messages lie in [0, 2p): otherwise FBS_E_INVALID, and nothing is written.  Explicit nonces stay below 2^55 (nonce0 +
 * G <= 2^55); fresh ones come from an atomic counter of the handle over [2^55, 2^56) (FBS_E_STATE when used up).  count = 0 does
 * nothing.  The entries up to fbs_pub_expand use no context and no GPU; libfbspublic.so (make -C tfhe_fbs_map_amd/csrc public: a
 * C++17 compiler, no ROCm) exports exactly those nine, and libfbsexec.so all of them. */
typedef struct fbs_pub fbs_pub;
int fbs_pub_key_words(const fbs_params *p, size_t *words);   /* k N */
/* sk_glwe [k][N] bits, as fbs_export_keys returns them (anything but 0 and 1: FBS_E_INVALID) -> bodies [k][N] */
int fbs_pub_keygen(const fbs_params *p, const uint8_t mask_key[32], const uint64_t *sk_glwe, const uint8_t noise_seed[32], uint64_t *bodies);
/* the encryptor's handle: the public key and the key its own randomness is expanded from.  One thread at a time, except that
 * fbs_pub_encrypt_fresh calls on several threads never share a stream. */
int fbs_pub_create(const fbs_params *p, const uint8_t mask_key[32], const uint64_t *bodies, const uint8_t seed[32], fbs_pub **out);
void fbs_pub_destroy(fbs_pub *pub);
/* text of the last failure on `pub`; NULL: of the thread's last failed entry that takes no handle (creation, keygen, word counts, expansion) */
const char *fbs_pub_last_error(const fbs_pub *pub);
int fbs_pub_words(const fbs_params *p, size_t count, size_t *words);   /* ceil(count / N) (k + 1) N */
int fbs_pub_encrypt(const fbs_pub *pub, const int64_t *msgs, size_t count, uint64_t nonce0, uint64_t *glwe);
int fbs_pub_encrypt_fresh(fbs_pub *pub, const int64_t *msgs, size_t count, uint64_t *glwe, uint64_t *nonce0);   /* *nonce0 (may be NULL): the first stream taken */
/* glwe [fbs_pub_words(count)] -> cts [count][D+1] on the host: the reference the device entries are held to */
int fbs_pub_expand(const fbs_params *p, const uint64_t *glwe, size_t count, uint64_t *cts);
/* libfbsexec.so only.  The same on device buffers, asynchronous on `stream` (NULL = the context's own), one kernel (k_expand_public)
 * that stages each sample's masks in LDS and writes whole ciphertexts, 16 bytes a lane; being device memory, the words cannot be
 * checked by the host.  Needs no key and no scratch. */
int fbs_pub_expand_dev(fbs_ctx *ctx, const uint64_t *d_glwe, size_t count, uint64_t *d_cts, void *stream);
/* Rows [row0, row0 + rows) of a state, flattened [row][sample] (j = r T + s, the order of fbs_state_fetch_packed), from the
 * G = ceil(rows T / N) samples at `glwe` in HOST memory.  Every word is checked on the host before anything is queued (FBS_E_INVALID,
 * state untouched); (k + 1) N G words cross the bus into staging that belongs to the context's scratch (repeated calls of one
 * shape do not grow it) and are expanded on the device into the rows.  Works on evaluation-only contexts and on contexts without
 * any key.  Blocks until done, as fbs_state_put. */
int fbs_state_put_public(fbs_ctx *ctx, fbs_state *st, size_t row0, size_t rows, const uint64_t *glwe);

/* ---- folded state: N resident bits in one full-precision GLWE sample, linked back in without a refresh ---------------------------
 * A full ciphertext costs D + 1 words per bit; a compact one has been through the key switch and pays a bootstrap to come back; a
 * packed output cannot come back at all.  A FOLD is a packing key switch taken straight from the big key: up to N big-key
 * ciphertexts go into the N coefficients of one GLWE sample under the same key, (k + 1) N words for N bits, with no rounding of
 * the result.  The sample is exactly what "public-key inputs" calls a sample, and fbs_pub_expand / fbs_pub_expand_dev turn it back
 * into big-key ciphertexts with no key at all (UNFOLD).  Its noise (params.folded_state_variance) never touches sigma_lwe, so the
 * unfolded ciphertexts enter the next program unrefreshed.  libfbsexec.so only.
 *
 * FOLD KEY, parameters (t_f, gamma_f), 1 <= t_f, 1 <= gamma_f, t_f gamma_f <= 31.  Rows (i, v), i < D = k N, v < t_f, layout
 * [D][t_f][k+1][N]: row (i, v) is a GLWE encryption of the constant polynomial s_i h_v, where s_i is word i of the flattened big key
 * -- the key bit under which word i of a big-key ciphertext's mask is read, the extraction convention of "public-key inputs" -- and
 * h_v = round(q / 2^(gamma_f (v+1))): polynomials A_0 .. A_(k-1), then B = sum_c A_c S_c + e + s_i h_v (e: sigma_glwe).  Row
 * r = i t_f + v takes its masks from stream (22, r) under the public mask key and its noise from stream (23, r) under the context's
 * key: two domains nothing else draws from, so every other key, ciphertext and known answer is word for word what it was.  Only
 * the bodies [D][t_f][N] travel.  The key belongs to the evaluation keys it was made beside: fbs_keygen, fbs_import_keys,
 * fbs_keygen_seeded and fbs_import_seeded_keys drop it, as they drop the packing key.
 *
 * FOLD.  Input: `count` big-key ciphertexts (a_j, b_j), in order; ciphertext j goes to coefficient j mod N of sample g = j / N; the
 * last sample may be partly filled.
 *   1. every mask word a in [0, q) to t_f gamma_f bits, q treated as 2^46: r = 46 - t_f gamma_f,
 *      a' = (((a >> (r-1)) + 1) >> 1) mod 2^(t_f gamma_f) -- the key switch's own rounding (the integer function its kernels
 *      compute before they add the digit offsets; in the sources, compact_round);
 *   2. a' into t_f BALANCED digits exactly as step 3 of PACKING;
 *   3. the body word b_j is used as it is: there is no lift;
 *   4. D_(i,v)(X) = sum_j d_v(a'_(j,i)) X^j;  ACC_c = - sum_(i,v) D_(i,v) A_c^(i,v)  (c < k),
 *      ACC_k = sum_j b_j X^j - sum_(i,v) D_(i,v) B^(i,v);  negacyclic, mod q; coefficients at and above the fill take b_j = 0.
 * There is NO transport rounding: a sample is its k + 1 polynomials as canonical residues, [k+1][N] words, the layout
 * fbs_pub_expand reads; a batch is its samples back to back, fbs_pub_words(count) words.  Every value is an exact residue: the
 * words do not depend on "pack_slices" (which cuts the i-sum here as it does for packing, at most min(32, D) ways) or launch shape.
 * UNFOLD is fbs_pub_expand / fbs_pub_expand_dev as they stand: the phase of ciphertext j is that of its source plus the fold's noise.
 *
 * Every entry writes nothing when it fails.  fbs_ctx_stat: "fold_key", "fold_levels", "fold_base_bits". */
/* Makes the fold key (on the device with "keys_on_device", else on the host) and uploads it in the transform domain.  FBS_E_STATE
 * unless the context's keys came from fbs_keygen_seeded on this context; FBS_E_INVALID for parameters outside the range above. */
int fbs_fold_keygen(fbs_ctx *ctx, uint32_t t_f, uint32_t gamma_f);
/* word counts for t_f levels (0: the context's own key; FBS_E_STATE without one): sizes[0] = D t_f N (bodies), sizes[1] = D t_f (k+1) N */
int fbs_fold_key_sizes(const fbs_ctx *ctx, uint32_t t_f, size_t sizes[2]);
/* bodies [D][t_f][N]; full (a test hook) the whole key [D][t_f][k+1][N] in the coefficient domain.  Either pointer may be NULL. */
int fbs_export_fold_key(const fbs_ctx *ctx, uint64_t *bodies, uint64_t *full);
/* The mirror: expands the masks from the context's mask key and uploads.  Works on evaluation-only contexts.  Every body word must
 * be a canonical residue (FBS_E_INVALID); a refused call leaves the previous fold key in place. */
int fbs_import_fold_key(fbs_ctx *ctx, uint32_t t_f, uint32_t gamma_f, const uint64_t *bodies);
/* d_cts [count][D+1] (any big-key ciphertexts, device) -> d_glwe [fbs_pub_words(count)] (device, 16-byte aligned: FBS_E_INVALID
 * otherwise), asynchronous on `stream`; needs no secret; FBS_E_STATE without a fold key.  Runs in passes of whole samples (8192
 * ciphertexts, one sample where N is larger); its scratch (the rounded fields of a pass, partial accumulators) is the packing
 * scratch and grows like any other: repeated calls of one shape do not grow it. */
int fbs_fold_dev(fbs_ctx *ctx, const uint64_t *d_cts, size_t count, uint64_t *d_glwe, void *stream);
/* Rows [row0, row0 + rows) of a resident state, flattened [row][sample] as fbs_state_fetch_packed flattens them, folded on the
 * device (word for word fbs_fold_dev of the full fetch); out [fbs_pub_words(rows T)] on the host.  Blocks until they are back. */
int fbs_state_fold(fbs_ctx *ctx, const fbs_state *st, size_t row0, size_t rows, uint64_t *out);
/* The same into a device buffer (16-byte aligned), queued on the context's stream like the other state entries. */
int fbs_state_fold_dev(fbs_ctx *ctx, const fbs_state *st, size_t row0, size_t rows, uint64_t *d_glwe);
/* The device-source twin of fbs_state_put_public: the samples at d_glwe (device) expanded into rows [row0, row0 + rows), no host
 * copy, no staging; being device memory, the words cannot be checked.  Queued on the context's stream; needs no key. */
int fbs_state_unfold_dev(fbs_ctx *ctx, fbs_state *st, size_t row0, size_t rows, const uint64_t *d_glwe);

/* ---- encrypted-index reads: rotate a folded table by an encrypted index -------------------------------------------------------------
 * A folded sample is a full-precision GLWE sample under the big key, the key the blind rotation works under, and its words are
 * canonical residues like a test polynomial's: it can BE the accumulator of a blind rotation.  Started from
 * (X^-b~ A_0, .., X^-b~ B) instead of the trivial (0, .., 0, X^-b~ TV), the rotation turns an encrypted table by an encrypted
 * amount, and sample extraction returns the entry.  libfbsexec.so only.
 *
 * BOX MAP, the box rule of the test polynomials: for coefficient j < N, slot(j) = floor((2 p j + N) / (2 N)).  slot(j) < p:
 * coefficient j carries entry slot(j).  slot(j) == p, the top half box: coefficient j carries MINUS entry 0 -- the half box below
 * X^N wraps negacyclically.
 *
 * TABLE: one GLWE sample, [k+1][N] canonical residues, the layout fbs_fold_dev writes; coefficient j of its phase is the phase of
 * the ciphertext the box map puts there.
 *
 * MAPPED FOLD.  map[j], j < count, names the source of fold position j: the low 31 bits an index into d_cts; bit 31
 * (FBS_MAP_NEG) set: the ciphertext is negated before anything else, every word, masks and body, x -> (q - x) mod q;
 * FBS_MAP_NONE: no ciphertext, zero words, as for positions past the fill.  The result is WORD FOR WORD fbs_fold_dev of the
 * materialised array: rounding, digits, slicing and passes are the fold's own.
 *
 * LOOKUP.  Input: an index ciphertext under the big key, and a table.
 *   1. key switch and modulus switch exactly as fbs_bootstrap_batch_dev runs them: (a~_1 .. a~_n, b~) in [0, 2N);
 *   2. the blind rotation, its initial accumulator component c = X^-b~ (polynomial c of the table), centred;
 *   3. sample extraction of coefficient 0; no constant is added.
 * With r = b~ - sum a~_i s_i mod 2N the output's phase is coefficient r of the table's for r < N and minus coefficient r - N for
 * r >= N.  An index of message x < p therefore reads entry x; an index with its padding bit set reads the NEGATED entry
 * (documented, not refused); the same holds for any table of at most p entries laid out by the box map.
 *
 * NOISE.  Rotating by a monomial adds nothing: the output's variance is v_br (table_out_norm2 + fold_factor + 1)
 * (params.lookup_output_norm2); the index is read like any refreshed full link (params.lookup_index_margin).
 *
 * Every entry writes nothing when it fails. */
#define FBS_MAP_NONE 0xFFFFFFFFu
#define FBS_MAP_NEG 0x80000000u
/* The box map of a table of `len` <= p entries, host side and pure: map_out[j], j < N, = base + slot(j) stride for slot(j) < len,
 * FBS_MAP_NONE for len <= slot(j) < p, and base | FBS_MAP_NEG for slot(j) == p (minus entry 0).  FBS_E_INVALID for p < 2, N not a
 * power of two in [2, 2^16], len == 0, len > p, or a source index that does not fit 31 bits. */
int fbs_lookup_map(uint32_t p, uint32_t N, uint32_t len, uint32_t base, uint32_t stride, uint32_t *map_out);
/* d_cts [n_src][D+1] and d_map [count] (device) -> d_glwe [fbs_pub_words(count)] (device, 16-byte aligned: FBS_E_INVALID
 * otherwise), asynchronous on `stream`, in the passes and on the scratch of fbs_fold_dev.  The map is device memory the host cannot
 * check: an index >= n_src that is not FBS_MAP_NONE reads source 0, never past the array.  n_src in [1, 2^31); needs no secret;
 * FBS_E_STATE without a fold key. */
int fbs_fold_mapped_dev(fbs_ctx *ctx, const uint64_t *d_cts, size_t n_src, const uint32_t *d_map, size_t count, uint64_t *d_glwe, void *stream);
/* d_tables [n_tables][k+1][N] (device, 16-byte aligned), d_cts_index [count][D+1] -> d_cts_out [count][D+1], the LOOKUP above,
 * asynchronous on `stream`.  d_table_of [count] (device) names each index's table, an id >= n_tables reading table 0; NULL: index i
 * reads table i.  Needs neither a secret nor a fold key. */
int fbs_lookup_dev(fbs_ctx *ctx, const uint64_t *d_tables, uint32_t n_tables, const uint32_t *d_table_of, const uint64_t *d_cts_index,
                   size_t count, uint64_t *d_cts_out, void *stream);
/* The same with the indices as compact ciphertexts d_words [count][W] at width `bits`: fbs_refresh_compact_dev with the table in
 * place of the identity polynomial, in that entry's passes and with its unpack.  At bits = log2(2N) the fields ARE the rotation
 * amounts. */
int fbs_lookup_compact_dev(fbs_ctx *ctx, const uint64_t *d_tables, uint32_t n_tables, const uint32_t *d_table_of, const uint64_t *d_words,
                           size_t count, uint32_t bits, uint64_t *d_cts_out, void *stream);
/* Resident state read by an encrypted index.  For every sample s < T of the index state and every plane m < n_planes, row
 * out_row0 + m of out_state at sample s is the entry, chosen by row `index_row` of index_state at sample s, of plane m's table.
 * axis = 0 (rows): plane m's entries are rows rows[m len .. m len + len) of table_state at sample s -- or, where table_state has
 * T = 1, at sample 0 for every s: one shared table per plane, folded once.  axis = 1 (samples): plane m's entries are samples
 * 0 .. len - 1 of row rows[m], shared by every query; len is table_state's T.  1 <= len <= p.  The box maps are made on the host and
 * uploaded once per call; the tables (T n_planes of them, n_planes where shared) are one mapped fold into a scratch of their own,
 * (k+1) N words a table, which grows like the others; the rotation is one launch sequence in which the planes of an index share its
 * key switch and modulus switch.  out_state has the index state's T and is neither of the other two.  Queued on the context's
 * stream like the other state entries; FBS_E_STATE without a fold key; needs no secret.
 * fbs_ctx_stat: "lookup_tables" (tables the last call folded), "lookup_scratch_words" (words of the table scratch). */
int fbs_state_lookup(fbs_ctx *ctx, const fbs_state *table_state, const uint32_t *rows, uint32_t n_planes, uint32_t len, uint32_t axis,
                     const fbs_state *index_state, size_t index_row, fbs_state *out_state, size_t out_row0);

/* ---- encrypted tables: the primitives of a write by an encrypted index -------------------------------------------------------------
 * A read takes entry i of a folded table by rotating the table by the index's amount r and extracting coefficient 0.  A WRITE adds
 * X^{+r} U to the table, U a folded sample that holds the value in the box of entry 0 and zero elsewhere: the same rotation kernels,
 * started from U, turned by the NEGATED amounts, with the whole rotated sample kept instead of one coefficient of it.
 * libfbsexec.so only.
 *
 * WIDE BOXES.  The amount a write turns by and the amount a later read of the same entry turns by differ by the index's noise, so
 * under the box map above (width N/p) a read can fall outside what a write covered.  A writable table gives an entry `spread` = s
 * ordinary boxes, and its index holds s i instead of i.  With W(c) = floor((2 p c + s N) / (2 s N)) for signed c in (-N, N) (floor
 * towards minus infinity), coefficient j < N of a table of len <= floor(p / s) entries takes
 *     entry W(j)                 where W(j) < len,
 *     MINUS entry 0              where W(j - N) == 0 (the half box of entry 0 below X^N),
 *     nothing                    elsewhere.
 * At s = 1 this is the box map, word for word; at len = 1 it is the unit box U of a write.  For s >= 2, any entries i, i' <
 * floor(p / s) and any amounts r_w, r_r that the box rule decodes to s i and s i': reading X^{r_w} U at r_r gives 1 if i = i' and 0
 * otherwise (tests/test_table_reference.py, exhaustively at small N) -- the index margin that admits a read admits a write at
 * spread 2.
 *
 * Every entry writes nothing when it fails. */
/* The map of a writable table, host side and pure: map_out[j], j < N, = base + W(j) stride, base | FBS_MAP_NEG or FBS_MAP_NONE as
 * above.  spread = 1 is fbs_lookup_map.  FBS_E_INVALID for p < 2, N not a power of two in [2, 2^16], spread < 1, len == 0,
 * len > floor(p / spread), or a source index that does not fit 31 bits. */
int fbs_table_map(uint32_t p, uint32_t N, uint32_t spread, uint32_t len, uint32_t base, uint32_t stride, uint32_t *map_out);
/* fbs_lookup_dev without its sample extraction: d_glwe_out [count][k+1][N] (device, 16-byte aligned) takes the WHOLE rotated sample
 * of every index, canonical residues, X^{-r} (its table) -- or, with FBS_ROTATE_NEGATE in `flags`, X^{+r} (its table): every one of
 * the n + 1 amounts of every row a -> (2N - a) mod 2N after the modulus switch (zero stays zero: skipped steps stay skipped).  Other
 * flag bits: FBS_E_INVALID.  Extracting coefficient 0 of an output without the flag gives fbs_lookup_dev's ciphertext, word for
 * word.  Needs neither a secret nor a fold key. */
#define FBS_ROTATE_NEGATE 1u
int fbs_rotate_dev(fbs_ctx *ctx, const uint64_t *d_tables, uint32_t n_tables, const uint32_t *d_table_of, const uint64_t *d_cts_index,
                   size_t count, uint32_t flags, uint64_t *d_glwe_out, void *stream);
/* The same with the indices as compact ciphertexts, as fbs_lookup_compact_dev takes them. */
int fbs_rotate_compact_dev(fbs_ctx *ctx, const uint64_t *d_tables, uint32_t n_tables, const uint32_t *d_table_of, const uint64_t *d_words,
                           size_t count, uint32_t bits, uint32_t flags, uint64_t *d_glwe_out, void *stream);
/* Sample dst_of[f] of d_dst [n_dst][k+1][N] += sample f of d_src [count][k+1][N], f < count, word by word modulo q (both device,
 * 16-byte aligned, canonical residues, and DISJOINT: overlapping arrays are FBS_E_INVALID), asynchronous on `stream`.  dst_of is
 * HOST memory [count] and is checked: a target >= n_dst
 * or a target named twice (two sums into one sample in one launch would race) is FBS_E_INVALID.  The upload of dst_of blocks.
 * Needs no key. */
int fbs_glwe_add_dev(fbs_ctx *ctx, uint64_t *d_dst, size_t n_dst, const uint32_t *dst_of, const uint64_t *d_src, size_t count, void *stream);

/* RESIDENT TABLES.  An fbs_table owns folded samples in device memory that persist until freed: fbs_state_lookup folds its tables
 * again on every call, a resident table is folded once, read by rotation and updated by rotation.  Tables are made of rows of a
 * resident state as at fbs_state_lookup, axis 0: plane m's entries are rows rows[m len .. m len + len) of `state`, at every sample s
 * of it -- n_planes T tables, table (m, s) being number m T + s -- or, where the state has T = 1, one SHARED table per plane.
 * Every entry below is queued on the context's stream like the state entries and needs no secret.
 *
 * WRITE, mode 0 (ADD): entry[index] += value, plain integer addition that must stay below p (the caller's bound).  The value of
 * table (m, s) is row value_rows[m] of value_state at sample s.  One key switch and modulus switch of the index; every value folded
 * into a unit box (fbs_table_map at len = 1); the boxes turned by the negated amounts, whole samples out; the sums into the
 * tables.  Mode 1 (SET): entry[index] = value.  First the old entry is read by the same amounts and refreshed through an ordinary
 * bootstrap by the identity table (without it a written box would carry twice the table's noise after every set), then value -
 * old is added as above.  `identity`: a table set of this context whose table 0 is the identity, or NULL for the context's own.
 * A shared table is written only by an index state of T = 1: several samples writing one table in one call have no order.
 *
 * NOISE (params.table_write_norm2): a written table carries table + value + fold_factor + 1 in units of the blind rotation's
 * variance, one more after a set; a read's output the table's + 1.
 * fbs_ctx_stat: "tables_alive", "table_scratch_words" (the write scratch: two samples and a ciphertext a table).  The unit-box
 * maps of the writes are made once by fbs_table_create, N words a table on the device; a write uploads a few words a table. */
typedef struct fbs_table fbs_table;
/* FBS_E_INVALID for spread < 1, len == 0, len > floor(p / spread), a row past the state; FBS_E_STATE without a fold key. */
int fbs_table_create(fbs_ctx *ctx, const fbs_state *state, const uint32_t *rows, uint32_t n_planes, uint32_t len, uint32_t spread,
                     fbs_table **out);
/* Waits for the work queued on the context, then frees.  NULL is allowed.  fbs_ctx_destroy frees the tables still alive. */
void fbs_table_free(fbs_table *table);
/* "tables", "planes", "samples" (T, or 1: shared), "len", "spread", "writes" (the writes that succeeded), "words" (tables (k+1) N). */
int fbs_table_stat(const fbs_table *table, const char *name, int64_t *value);
/* Every table, [tables][k+1][N] words, to the host (for tests, and for saving a table); blocks. */
int fbs_table_words(fbs_ctx *ctx, const fbs_table *table, uint64_t *out);
/* Row out_row0 + m of out_state at sample s <- the entry of table (m, s) -- of plane m's shared table -- that row index_row of
 * index_state names at sample s: fbs_state_lookup's rotation without its fold; the planes share the index's one key switch.  The
 * index state has the tables' T (any T where they are shared); out_state has the index state's T and is another state. */
int fbs_table_read(fbs_ctx *ctx, const fbs_table *table, const fbs_state *index_state, size_t index_row, fbs_state *out_state,
                   size_t out_row0);
/* value_rows [n_planes].  The tables are untouched when the call fails. */
int fbs_table_write(fbs_ctx *ctx, fbs_table *table, const fbs_state *index_state, size_t index_row, const fbs_state *value_state,
                    const uint32_t *value_rows, uint32_t mode, const fbs_tvset *identity);

/* ---- a loaded program, one level at a time (multi-GPU hosts) -----------------
 * The two independent axes of the reference's eval loop (fbs_exec_env.py:211-223) are the gates
 * of a bootstrap level and the samples.  A host that shards the GATES of a level over several
 * GPUs keeps a replicated wire buffer per GPU, [n_slots][T][D+1] words of its own device
 * memory, and steps the program with the calls below; every index array they need was
 * uploaded by fbs_program_load, so each call is a few kernel launches on `stream` and
 * nothing else.  Wires live in SLOTS: a wire's slot is reused once its last reader has run,
 * so n_slots is the peak number of live wires, not the number of wires.
 *   level L in [0, n_levels]:  fbs_level_lincomb_dev    the LinearProds of level L
 *   level L in [0, n_levels):  fbs_level_bootstrap_dev  bootstraps f in [f_begin, f_end) of the
 *        level's [n_gates][s_count] grid (gate-major), each preceded by the key switch of its
 *        source -- one key switch per distinct (source wire, sample), shared by the gates that
 *        read it.  d_rows == NULL: results go to their wire slots; else to row f - f_begin of
 *        d_rows ([f_end - f_begin][fbs_layout.row_words], e.g. the send buffer of an all-gather), and
 *   fbs_level_scatter_dev copies rows of such an array (after the all-gather) into the slots.
 * Samples [s_begin, s_begin + s_count) of every wire are processed; T is the sample stride. */
typedef struct fbs_layout {
    uint32_t n_slots;      /* wire slots a wire buffer needs                                   */
    uint32_t n_levels;     /* bootstrap levels                                                 */
    uint32_t max_width;    /* bootstraps in the widest level                                   */
    uint32_t max_sources;  /* key switches in the level that has most                          */
    uint32_t n_bootstrap;  /* bootstraps in the program                                        */
    uint32_t n_keyswitch;  /* key switches in the program (<= n_bootstrap: shared sources)     */
    uint32_t n_inputs, n_outputs;
    uint32_t n_rotations;  /* blind rotations per sample (< n_bootstrap when tables share them)       */
    uint32_t row_words;    /* words per row of the d_rows arrays below: D + 1, or (k + 1) N for a fused program */
} fbs_layout;
int fbs_program_layout(const fbs_prog *prog, fbs_layout *out);
int fbs_program_level(const fbs_prog *prog, uint32_t level, uint32_t *n_gates, uint32_t *n_sources);
/* in_slot[n_inputs]: where input i is expected; out_slot[n_outputs]: slot of output o, or -1-c for a constant c */
int fbs_program_io_slots(const fbs_prog *prog, uint32_t *in_slot, int64_t *out_slot);
int fbs_level_lincomb_dev(fbs_ctx *ctx, const fbs_prog *prog, uint32_t level, uint64_t *d_wires, size_t T,
                          size_t s_begin, size_t s_count, void *stream);
int fbs_level_bootstrap_dev(fbs_ctx *ctx, const fbs_prog *prog, uint32_t level, uint64_t *d_wires, size_t T,
                            size_t s_begin, size_t s_count, size_t f_begin, size_t f_end, uint64_t *d_rows,
                            void *stream);
int fbs_level_scatter_dev(fbs_ctx *ctx, const fbs_prog *prog, uint32_t level, uint64_t *d_wires, size_t T,
                          size_t s_begin, size_t s_count, const uint64_t *d_rows, size_t f_begin, size_t f_end,
                          void *stream);

/* ---- audited evaluation: the noise of a stepped program, measured where its margin is defined -------------------------------
 * Between the level calls above, fbs_audit_level_dev turns the ciphertexts of one point of one level, plus the cleartext value
 * each should hold, into exact error statistics on the device (fbs_audit.hip), under the secret keys the context keeps there.
 * Two units:
 *   wire units   (INPUTS, LINCOMB, BOOTSTRAP): big-key ciphertexts in their wire slots.  phase = b - <a, S> mod q;
 *                e = centred((phase - Delta m) mod q) with m = expected mod 2p and Delta = 2 round(q / 4p): an integer in
 *                [-(q-1)/2, (q-1)/2], the torus error is e / q, and a sample is `over` when 4p |e| >= q.
 *   field units  (ROTATION_INPUT): the (n + 1) fields of log2(2N) bits that the key switch and the modulus switch leave for the
 *                blind rotation.  ph = body - <mask, s> mod 2N; e = centred((2p ph - 2N m) mod 4pN) in [-2pN, 2pN): the torus
 *                error is e / (4pN), the half box is N, and a sample is `over` when |e| >= N.  (2p Delta stands for q here: a
 *                relative difference of at most 4p / q.)
 * `over` is a half-box criterion, not a comparison of decoded messages: an error of half a box or more is what makes a blind
 * rotation land in a neighbouring box, whatever the table then returns there.
 * FBS_AUDIT_ROTATION_INPUT runs the same key switch, at the same width log2(2N), that fbs_level_bootstrap_dev(level) runs over
 * the level's full range, into the same scratch, and decodes that scratch; the key switch is deterministic, so these are the very
 * words the rotation reads.  It must be called after fbs_level_lincomb_dev(level) and before fbs_level_bootstrap_dev(level): a
 * source's slot may be reused by the level's own outputs.  Likewise INPUTS before level 0 runs, LINCOMB(level) right after
 * fbs_level_lincomb_dev(level) and BOOTSTRAP(level) right after fbs_level_bootstrap_dev(level) (into the wire slots).  LINCOMB
 * reports the LinearProds of the level whose slot still holds them when the level's LinearProds have all run (a wire nobody
 * outside an earlier sub-stage reads may have lent its slot to a later one).  BOOTSTRAP of a fused program reports the outputs
 * of the level's own rotations, then those cut out of shared rotations.
 * Errors: FBS_E_STATE on a context without a secret (evaluation-only); FBS_E_INVALID for a level the point does not have
 * (LINCOMB: [0, n_levels]; ROTATION_INPUT, BOOTSTRAP: [0, n_levels)), an unknown point, a bad sample range, more than 2^18
 * samples in one call (the bound under which the 64-bit sum and the 128-bit sum of squares cannot overflow: |e| < 2^45), or null
 * pointers with n_rows * s_count > 0.  s_count = 0 does nothing.  The statistics are exact integers, computed without floating
 * point or atomics: the same inputs give the same words. */
#define FBS_AUDIT_INPUTS          0u  /* the input slots (level ignored)                               : wire units   */
#define FBS_AUDIT_LINCOMB         1u  /* wires the LinearProds of level L write                        : wire units   */
#define FBS_AUDIT_ROTATION_INPUT  2u  /* the level's distinct key-switch sources, after KS + MS        : field units  */
#define FBS_AUDIT_BOOTSTRAP       3u  /* wires the Bootstraps of level L write                         : wire units   */
typedef struct fbs_audit_row { uint64_t count, over, max_abs; int64_t sum; uint64_t sumsq_lo, sumsq_hi; } fbs_audit_row;

/* rows of (level, point) and the PROGRAM WIRE ID (fbs_program_desc numbering) of each, in the order the audit reports them */
int fbs_audit_rows(const fbs_prog *prog, uint32_t level, uint32_t point, uint32_t *n_rows, uint32_t *wire_ids /* may be NULL */);
/* d_expected: device [n_rows][s_count] int64, the cleartext value of each row's wire per sample (any integer; taken mod 2p).
 * stats: host [n_rows]; errors: host [n_rows][s_count] or NULL.  Blocks until they are back. */
int fbs_audit_level_dev(fbs_ctx *ctx, const fbs_prog *prog, uint32_t level, uint32_t point, const uint64_t *d_wires, size_t T,
                        size_t s_begin, size_t s_count, const int64_t *d_expected, fbs_audit_row *stats, int64_t *errors, void *stream);

/* ---- measurement hooks ------------------------------------------------------
 * When enabled, every kernel launch is bracketed by HIP events on its own
 * stream; fbs_profile_read synchronises and returns per-kernel totals since the
 * last reset: ms[0]=keyswitch+modswitch, ms[1]=blind-rotate+extract, ms[2]=lincomb;
 * launches[i] = number of launches. */
int fbs_profile_enable(fbs_ctx *ctx, int on);
int fbs_profile_read(fbs_ctx *ctx, double ms[3], uint64_t launches[3], int reset);
/* name of the kernel instantiation the most recent launch of kind `which` (0, 1, 2 as above) used: the launcher
 * picks the shape by parameter set and batch size */
const char *fbs_profile_kernel(const fbs_ctx *ctx, int which);
/* The same totals per kernel instantiation since the last reset (fbs_profile_read with reset clears them too): lines
 * "<kind>\t<kernel>\t<launches>\t<ms>\n", kind = 0, 1, 2 as above.  A launch the launcher cuts into a whole-round part and
 * a remainder shows as two entries.  *needed (may be NULL) = bytes the text takes; buf == NULL only asks for that. */
int fbs_profile_kernels(fbs_ctx *ctx, char *buf, size_t cap, size_t *needed);
/* newline-separated names of every key-switch and blind-rotation kernel instantiation the launchers can pick, by the
 * rules of their dispatch: what tests/test_gpu_dispatch.py drives one by one against the oracle */
const char *fbs_kernel_catalog(void);
/* block until all work queued on the context's stream (or `stream`) has finished */
int fbs_sync(fbs_ctx *ctx, void *stream);

/* ---- mapper: coefficient search ------------------------------------
 * Stands behind MapToFBSHeur._find_lincomb_coefs_search (fbs_mapper/map_to_fbs.py:363-392): x, y are the multi-value
 * columns of two cones over the `rows` rows of their joint truth table (xy_mvt[:, 0], xy_mvt[:, 1]), tt the merged output
 * bit per row (r_tt).  On success *found says whether a legal (a, b) exists; then ab = {a, b} and, if mvt != NULL,
 * mvt[r] = a x[r] + b y[r] -- the reference's (r_ab, r_mvt), chosen by the reference's rule among the reference's
 * candidates.  Needs no keys: a searcher is bound to a device only.  max_fbs_size <= 128. */
typedef struct fbs_searcher fbs_searcher;
int fbs_searcher_create(int device, fbs_searcher **out);
void fbs_searcher_destroy(fbs_searcher *s);
const char *fbs_searcher_last_error(const fbs_searcher *s);
/* device time of the most recent search kernel (HIP events on the searcher's stream), ms */
double fbs_searcher_last_kernel_ms(const fbs_searcher *s);
int fbs_search_lincomb_coefs(fbs_searcher *s, const int32_t *x, const int32_t *y, const uint8_t *tt, uint32_t rows,
                             uint32_t fbs_size, uint32_t max_fbs_size, int32_t ab[2], int64_t *mvt, int *found);

/* ---- debug hook: negacyclic product of two polynomials on the device NTT ---- */
int fbs_debug_polymul(fbs_ctx *ctx, const uint64_t *a, const uint64_t *b, uint64_t *c);
/* ---- test hooks: the device's FP64 field primitives and its transforms in isolation (tests/test_gpu_transforms.py) ----
 * fbs_debug_field: element-wise over `count` int64 words holding integers |x| < 2^53 (w: the second operand of op 0 and 1, else
 * NULL); out[i] is the RAW result as an integer -- the exact representative, not its residue.  op: 0 fp_mulmod(x, w),
 * 1 fp_mulmod_exact(x, w), 2 fp_center(x), 3 fp_canon(x), 4 fp_canon_near(x), 5 fp_to_u64(fp_from_u64(x)) (0 <= x < 2^52). */
int fbs_debug_field(fbs_ctx *ctx, int op, const int64_t *x, const int64_t *w, size_t count, int64_t *out);
/* The rounded Gaussian (sampler 1) alone, on raw windows a test supplies -- edge inputs no ChaCha20 stream would hit: out[i] = the
 * sample of the six words words[6 i .. 6 i + 5] at standard deviation `sigma` (<= q, else FBS_E_INVALID; at most 2^26 windows).
 * Both work whatever the context's own sampler.  fbs_debug_gauss runs on the host and reads no context (ctx may be NULL; it only
 * takes the error text); fbs_debug_gauss_dev runs one kernel over `count` on device arrays, asynchronous on `stream`, and returns
 * the same words.  libfbsexec.so only. */
int fbs_debug_gauss(const fbs_ctx *ctx, const uint64_t *words, size_t count, uint64_t sigma, int64_t *out);
int fbs_debug_gauss_dev(fbs_ctx *ctx, const uint64_t *d_words, size_t count, uint64_t sigma, int64_t *d_out, void *stream);
/* The packing kernels alone (steps 2 - 5 and the transport of "packed outputs"), on fields a test supplies -- mask fields no key
 * switch under seeded keys can be made to give: d_fields [count][n + 1] uint32 below 2^31 (device), laid out as step 1 leaves them,
 * -> d_words [fbs_packed_words], asynchronous on `stream`.  No key switch, so a packing key is all it needs; rows past `count` are
 * not read.  Refuses what fbs_pack_dev refuses and, with FBS_E_INVALID, more than one pass of it (max(8192, the modulus-switch
 * scratch) ciphertexts, cut down to whole samples).  libfbsexec.so only (tests/test_gpu_pack_shapes.py). */
int fbs_debug_pack_fields_dev(fbs_ctx *ctx, const uint32_t *d_fields, size_t count, uint32_t bits, uint64_t *d_words, void *stream);
/* The front kernel of "folded state" alone (step 1 and the transposition): d_cts [count][D+1] -> d_fields, [D][cols] uint32 mask
 * words rounded to tg bits, then cols 64-bit body words (8-byte aligned; (D + 2) cols uint32 in all); cols a multiple of N,
 * count <= cols; columns past `count` are zero and the ciphertexts behind `count` are not read.  Needs no key.  libfbsexec.so only. */
int fbs_debug_fold_front_dev(fbs_ctx *ctx, const uint64_t *d_cts, size_t count, uint32_t cols, uint32_t tg, uint32_t *d_fields, void *stream);
/* Static text, no GPU needed: one line per transform variant some blind-rotation kernel instantiates, made from the lists the
 * kernels are instantiated from:
 *   "class=<PolyNtt|SplitNtt|WavesNtt|LaneNtt256|LaneNtt512> logn=<log2 N> lanes=<threads per polynomial> dir=forward first=<FIRST>[ np=<NP>]"
 *   "class=... logn=... lanes=... dir=inverse bounded=<0|1>"
 * (np: the polynomials LaneNtt*::forward_multi takes side by side; logn of a lane transform: the polynomial its four parts make). */
const char *fbs_debug_transform_list(void);
/* One workgroup per polynomial (per np polynomials) runs the call the kernels make, on a line of the list above; the context
 * must be of the variant's N (FBS_E_INVALID otherwise; the twiddle tables depend on N alone, so any k serves), polys a multiple of np.
 * int64 in and out, not reduced.  Coefficient side: natural order (a lane transform: its four parts back to back, each in natural
 * order).  Evaluation side: register order, word t*E + m = register m of thread t, E = N / lanes -- what forward leaves in a word
 * is what inverse takes from it; which evaluation point a word holds is found by transforming the monomial X.
 * One line is accepted without being listed: "class=SplitNtt logn=10 lanes=64 dir=inverse bounded=1 centre=exit", the inverse
 * k_blind_rotate takes where a wave holds a whole N = 1024 polynomial (SplitNtt::inverse_exit_centred: the residues of the listed
 * "bounded=1" line, other representatives). */
int fbs_debug_transform(fbs_ctx *ctx, const char *variant, const int64_t *in, int64_t *out, size_t polys);
/* ---- test hook: raises a C++ exception INSIDE the library (kind 0 std::bad_alloc, 1 std::length_error, 2 std::runtime_error,
 * 3 a non-standard one; else nothing) to show that none crosses this boundary: returns FBS_E_NOMEM, FBS_E_NOMEM,
 * FBS_E_INVALID, FBS_E_INVALID, FBS_OK, with the text in fbs_last_error(ctx) (ctx may be NULL: no device is touched). */
int fbs_debug_raise(fbs_ctx *ctx, int kind);

#ifdef __cplusplus
}
#endif
#endif /* FBS_EXEC_H */

// Internal definitions shared by the host side (fbs_host.cpp, fbs_capi.cpp, fbs_eval.cpp, fbs_client_entries.cpp) and the HIP
// side (fbs_kernels.hip) of libfbsexec.so -- and, with FBS_HOST_ONLY defined, by the client library libfbsclient.so
// (fbs_error.cpp, fbs_host.cpp, fbs_client_entries.cpp, fbs_client_capi.cpp), which is built without HIP: it then sees the host
// state of a context (fbs::HostState) and the host functions, and nothing that names a device type.
#pragma once
#ifndef FBS_HOST_ONLY
#include <hip/hip_runtime.h>
#endif

#include <atomic>
#include <cstdint>
#include <functional>
#include <map>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/fbs_exec.h"
#include "fbs_field.hpp"
#include "fbs_select.hpp"

namespace fbs {

// ---- randomness: ChaCha20 keyed by the context seed (spec in DESIGN.md) -----------------------
// Domains 9 and up are the seeded path's (fbs_keygen_seeded, fbs_encrypt_seeded): its masks are drawn under the public mask
// key (mask_key_of), its noise and secrets under the context's key.  No (key, stream) pair of the seeded path may equal one that
// fbs_keygen or fbs_encrypt uses, above all for noise: two key sets under one secret and one noise stream have bodies that differ
// by exactly (A - A') S, which gives the secret away.  The secret keys themselves are shared (DOM_SK_*), so that one client
// context can mix seeded and full calls.
enum Domain : uint64_t {
    DOM_SK_LWE = 1, DOM_SK_GLWE = 2, DOM_BSK_MASK = 3, DOM_BSK_NOISE = 4,
    DOM_KSK_MASK = 5, DOM_KSK_NOISE = 6, DOM_ENC_MASK = 7, DOM_ENC_NOISE = 8,
    DOM_MASK_KEY = 9,                                   // under the context's key: block 0 of stream 0 -> the public mask key
    DOM_SBSK_MASK = 10, DOM_SBSK_NOISE = 11,            // seeded bootstrapping key: mask (mask key), noise (context key)
    DOM_SKSK_MASK = 12, DOM_SKSK_NOISE = 13,            // seeded key-switching key
    DOM_SENC_MASK = 14, DOM_SENC_NOISE = 15,            // seeded encryption
    DOM_PACK_MASK = 16, DOM_PACK_NOISE = 17,            // packing key (packed outputs): mask (mask key), noise (context key)
    // public-key inputs (fbs_public.cpp; include/fbs_exec.h, "public-key inputs"): the public key's masks (mask key) and noise
    // (the key holder's noise seed); the encryptor's binary u and its noise, both under the encryptor's own key
    DOM_PUB_MASK = 18, DOM_PUB_NOISE = 19, DOM_PUB_ENC_U = 20, DOM_PUB_ENC_NOISE = 21,
    DOM_FOLD_MASK = 22, DOM_FOLD_NOISE = 23             // fold key (folded state): mask (mask key), noise (context key)
};
FBS_HD uint64_t stream_id(Domain d, uint64_t sub) { return ((uint64_t)d << 56) | (sub & 0x00FFFFFFFFFFFFFFull); }
// the 256-bit ChaCha key of a context: a 64-bit seed followed by a fixed tail (fbs_ctx_create: reproducible, test-grade), or
// derived from 32 caller-supplied bytes and the parameter set (fbs_ctx_create_seeded)
struct RandKey {
    uint32_t w[8];
};
RandKey rand_key_from_seed64(uint64_t seed);
RandKey rand_key_derive(const uint8_t seed[32], const fbs_params &p);
void rand_words(const RandKey &key, uint64_t stream, uint64_t idx0, uint64_t *dst, size_t count);
// `sampler`: fbs_params.sampler of the context the draw belongs to (fbs_sampler.hpp)
int64_t noise_sample(const RandKey &key, uint64_t stream, uint64_t idx, uint64_t sigma, uint32_t sampler = 0);
// The two samples every key and ciphertext is made of (fbs_host.cpp); a caller adds its message.
// mask_words: dst[i] = fold(word idx0 + i of (key, stream)), i < len.  lwe_body: noise sample 0 + sum_{sk_i = 1} mask_i.
void mask_words(const RandKey &key, uint64_t stream, uint64_t idx0, uint64_t *dst, size_t len);
uint64_t lwe_body(const RandKey &noise_key, uint64_t noise_stream, uint64_t sigma, uint32_t sampler, const uint64_t *mask,
                  const uint64_t *sk, size_t len);
// acc += a * S (negacyclic, S binary, given by its support)
void add_times_key(uint64_t *acc, const uint64_t *a, const std::vector<uint32_t> &support, uint32_t N);
// GLWE zero sample under the key of k = support.size() polynomials: masks [k][N], column c = mask_words at c N (the caller's row,
// or scratch when only the body is kept); body [N] = noise samples 0 .. N - 1 + sum_c A_c S_c
void glwe_zero_sample(const RandKey &mask_key, uint64_t mask_stream, const RandKey &noise_key, uint64_t noise_stream, uint64_t sigma,
                      uint32_t sampler, const std::vector<std::vector<uint32_t>> &support, uint32_t N, uint64_t *masks, uint64_t *body);
// test hooks of the rounded Gaussian (fbs_debug_gauss, fbs_debug_gauss_dev): what both refuse (null: nothing), and the host loop
const char *debug_gauss_refused(const void *words, size_t count, uint64_t sigma, const void *out);
void host_debug_gauss(const uint64_t *words, size_t count, uint64_t sigma, int64_t *out);
// the public mask key of the seeded path: the first four 64-bit words of chacha_block(key, stream_id(DOM_MASK_KEY, 0), 0),
// little-endian (ChaCha20 is a PRF keyed by `key`: publishing this block reveals nothing about it)
RandKey mask_key_of(const RandKey &key);

// launcher knobs (fbs_ctx_tune): which kernel shape a launch takes (fbs_select.cpp).  Defaults are the measured choices; tests
// use them to reach every instantiation at small sizes.
struct Tune {
    int64_t ks_mfma = 1;            // 0: never the GEMM
    int64_t ks_fp = 1;              // 0: integer kernels instead of the FP64 one (fallback path)
    int64_t br_cu_kernel = 1;       // 0: no one-bootstrap-per-CU kernel (the generic kernel on the four-wave transform instead)
    int64_t br_cu_lean = 1;         // 1: between one and two per CU, its 128-register variant (two workgroups per CU); 2: always; 0: never
    int64_t br_k2_shape = 0;        // k = 2: 0 by launch size; 3 always three waves per bootstrap; 12 always the twelve-wave latency shape
    int64_t br_glwe_fpw = 0;        // k_blind_rotate_glwe: bootstraps per workgroup -- 0 by launch size; 1, 2; anything larger = the throughput shape
    int64_t pack_slices = 0;        // packed outputs: slices the i-sum of one packed sample is cut into -- 0 by launch size (fbs_pack.hip)
    int64_t keys_on_device = 0;     // 1: the evaluation keys are made and expanded on the device (fbs_keygen.hip), not on the host
};

// ---- launch descriptors ------------------------------------------------------------------------
// A "gate" is one Bootstrap instruction applied to `s_count` samples of its source wire.  The bootstraps of a launch
// are the flattened indices f in [f_begin, f_begin + count) of the [n_gates][s_count] grid: gate g = f / s_count,
// sample s = s_begin + f % s_count.  Wire slot w, sample s lives at base + (w*T + s)*ct_words words.  Slot arrays may
// be null (identity), which is the plain batch API.
struct GateView {
    const uint64_t *in_base;
    uint64_t *out_base;
    const uint32_t *src_slot;   // [n_sources] or null: wire slot of key-switch source u
    const uint32_t *dst_slot;   // [n_gates] or null
    const uint32_t *table_ids;  // [n_gates] or null (table 0)
    // Gates that read the same wire share ONE key switch + modulus switch (reference fbs_mapper/map_to_fbs.py:41-45
    // emits several tables per linear combination): source_of[g] = index of gate g's source in src_slot, null = g.
    const uint32_t *source_of;  // [n_gates] or null
    uint64_t *out_rows;         // non-null: bootstrap f writes row (f - f_begin) of this contiguous array instead of its slot
    uint32_t row_words;         // words per row of out_rows; 0 = one ciphertext (D + 1).  2N for a fused level cut across GPUs:
                                // a shared rotation then leaves its whole accumulator in its row (it travels with the gather)
    // Several tables on ONE blind rotation (fused programs, fbs_program_load_ex): a gate whose dst_slot has bit 31 set is
    // the rotation of the table-independent test vector TV_0 for a source that several tables read; it leaves its whole
    // accumulator in row (dst & 0x7fffffff) * s_count + sample of acc_rows ([row][k + 1][N]) for k_multi_extract.
    uint64_t *acc_rows;
    size_t T;                   // samples per wire in the buffers (stride)
    size_t s_begin, s_count;    // sample window of the launch
    size_t f_begin, count;      // bootstraps of this launch (flattened gate-major over the window)
    size_t ks_begin, ks_count;  // key switches of this launch, flattened the same way over [n_sources][s_count];
                                // row r of the modulus-switched scratch holds flattened source index ks_begin + r
    uint32_t n_gates;
};

// Rows of ciphertexts for the device encryption and decryption (fbs_io.hip): ciphertext (r, s), r < rows, s < per_row, lives at
// cts + (slot * ct_stride + s) * (D + 1) with slot = row_slot[r] (row_slot null: slot = r; for decryption 0xFFFFFFFF = a row
// nobody touches), its message at msgs[r * msg_stride + s].
struct IoView {
    int64_t *msgs;   // (read by the encryption; the seeded expansion reads its bodies here, as uint64 words)
    size_t msg_stride;
    uint64_t *cts;   // (read by the decryption)
    const uint32_t *row_slot;
    size_t ct_stride;
    size_t rows, per_row;
};

// The device-side inputs and outputs of a chunk (fbs_state.hip): link e of a launch joins wire slot `slot`, samples q < tc, and the
// ciphertexts of samples s0 + q of a call; the side a link does not have is the trivial ciphertext (0, .., 0, body).  Loading,
// sample q comes from `row` (sample 0 of a state row, [T_src][D + 1] words) at sample index[s0 + q] -- `index` is the call's whole
// map on the device, [T] words, checked by the host against T_src; null is the identity -- and, where there is no row or the entry
// is FBS_SAMPLE_NONE, is the trivial ciphertext of msgs[q] (the chunk's plaintext messages on the device; null: of `body`, a
// residue worked out on the host).  Storing, sample s0 + q of `row` takes the slot's sample q, or -- slot WIRE_NO_SLOT, a constant
// output -- the trivial ciphertext of `body`; `index` and `msgs` are not read.  Every member is 8 bytes.
constexpr uint64_t WIRE_NO_SLOT = ~0ull;
struct WireLink {
    uint64_t *row;
    const uint32_t *index;
    const int64_t *msgs;
    uint64_t body;
    uint64_t slot;
};
struct WireCopy {
    const WireLink *links;   // [n_links], device
    size_t n_links;
    uint64_t *wires;         // wire slots [n_slots][Tc][D + 1]
    size_t Tc;               // samples per slot in the wire buffer (stride)
    size_t s0, tc;           // sample q < tc of a slot is sample s0 + q of the call
    uint32_t D;
    uint64_t delta;          // 2 round(q / 4p): a message m in [0, 2p) is the body m delta mod q (read by the load)
};

// The group sum (fbs_state.hip): sample j < T_dst of row r < rows of dst ([T_dst][D + 1] words a row) becomes the word-wise sum modulo q of samples
// [j group, min((j + 1) group, T_src)) of row r of src
struct SumGroups {
    const uint64_t *src;   // sample 0 of the first row read
    uint64_t *dst;         // sample 0 of the first row written
    size_t rows, T_src, T_dst, group;
    uint32_t D;
};

#ifndef FBS_HOST_ONLY
struct Profile {
    struct Pending {
        hipEvent_t begin, end;
        std::string kernel;   // instantiation the bracketed launch used
    };
    struct PerKernel {
        double ms = 0;
        uint64_t launches = 0;
    };
    bool on = false;
    std::vector<Pending> pending[3];
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pool;
    double ms[3] = {0, 0, 0};
    uint64_t launches[3] = {0, 0, 0};
    std::string kernel[3];   // instantiation of the most recent launch of each kind
    // the same totals per kernel instantiation: a launch that is cut into a whole-round part and a remainder shows as two entries
    std::map<std::string, PerKernel> by_kernel[3];
};
#endif

// The host state of a context: everything fbs_host.cpp reads or writes -- parameters and what is derived from them, the random
// keys, the nonce counter, the secrets and the host copies of the keys, the packing key's parameters and bodies, the error
// text.  No device type in it: the client library's context is this and nothing more, the GPU library's adds the device side.
struct HostState {
    fbs_params p{};
    uint64_t seed = 0;
    RandKey rkey{};                    // what all randomness of the context is expanded from
    mutable std::atomic<uint64_t> next_nonce{1ull << 55};  // fbs_encrypt_fresh: first unused encryption stream of [2^55, 2^56); reserved by compare-exchange
    uint32_t N = 0, D = 0, rows = 0;   // D = k*N, rows = (k+1)*l
    uint32_t group = 1;                // key bits per blind-rotation step (1 or 2)
    size_t n_ggsw = 0;                 // GGSW samples in the bootstrapping key: n, or 3n/2 for group 2
    uint32_t ksk_stride = 0;           // padded n+1
    uint64_t delta_half = 0;
    uint64_t g[16]{};                  // round(q / B^(lv+1))
    uint64_t h[64]{};                  // round(q / 2^(gamma (v+1)))
    mutable std::string err;

    bool have_keys = false;
    std::vector<uint64_t> sk_lwe, sk_glwe, bsk, ksk;   // host copies, standard layout
    // Seeded path: masks are drawn under `mask_key` (mask_key_of(rkey), or the one fbs_import_seeded_keys received).
    // seeded_keys: the evaluation keys came from fbs_keygen_seeded or fbs_import_seeded_keys; eval_only: they came from
    // fbs_import_seeded_keys, and the context holds no secret (sk_lwe, sk_glwe empty, d_sk_bits freed).
    RandKey mask_key{};
    bool seeded_keys = false, eval_only = false;

    // Packed outputs and folded state: the parameters and bodies [rows][t][N] of each gadget key (the masks come from mask_key)
    struct GadgetKeyState {
        bool have = false;
        uint32_t t = 0, gamma = 0;
        std::vector<uint64_t> bodies;
    } gadget[2];   // [GadgetKind]
};

// The gadget keys: rows x t GLWE encryptions under the big key of the constants src[i] h_v, i < rows, v < t.  Row r = i t + v:
// masks A_c = fold(words c N .. of stream (mask_dom, r)) under the mask key, body = e + sum_c A_c S_c + src[i] h_v at X^0, e on
// stream (noise_dom, r) under the context's key.  The packing key (packed outputs, fbs_pack.hpp) is the case src = sk_lwe,
// rows = n; the fold key (include/fbs_exec.h, "folded state") the case src = sk_glwe (the flattened big key itself), rows = D.
// What differs between the two is this table, gadget_rows and gadget_secret, and the device secret in dev_gadget_bodies.
enum GadgetKind { GK_PACK = 0, GK_FOLD = 1 };
struct GadgetKindInfo {
    const char *noun, *letter;   // what the entries and their messages call the key and its parameters (t_p, gamma_f)
    Domain mask_dom, noise_dom;
};
constexpr GadgetKindInfo GADGET_KINDS[2] = {{"packing", "p", DOM_PACK_MASK, DOM_PACK_NOISE}, {"fold", "f", DOM_FOLD_MASK, DOM_FOLD_NOISE}};
// a mapped fold's map entries (include/fbs_exec.h, "encrypted-index reads"): no ciphertext; the ciphertext negated
constexpr uint32_t FOLD_MAP_NONE = 0xFFFFFFFFu, FOLD_MAP_NEG = 0x80000000u;
inline uint32_t gadget_rows(const HostState &c, GadgetKind kind) { return kind == GK_PACK ? c.p.n : c.D; }
inline const std::vector<uint64_t> &gadget_secret(const HostState &c, GadgetKind kind) { return kind == GK_PACK ? c.sk_lwe : c.sk_glwe; }

}  // namespace fbs

#ifdef FBS_HOST_ONLY
struct fbs_ctx : fbs::HostState {};
#else
struct fbs_ctx : fbs::HostState {
    fbs::Tune tune;
    int64_t scratch_growths = 0;       // how often a call had to (re)allocate scratch, i.e. blocked (fbs_ctx_stat)
    int device = 0;
    std::string devinfo;
    int cu_count = 0;
    hipStream_t stream = nullptr;

    uint64_t *d_bsk_hat = nullptr;   // [n][rows][k+1][N]  NTT domain, lane-interleaved, x N^-1
    uint64_t *d_bsk_hat_small = nullptr;   // the same in the evaluation order of the small-launch shape (fbs_ntt.hpp), where small_key_needed
    uint64_t *d_ksk = nullptr;       // [D*t][ksk_stride]
    uint64_t *d_ksk_f = nullptr;     // the same key as centred doubles (bit patterns), for the FP64 key-switch kernel
    int8_t *d_ks_b = nullptr;        // the key as balanced base-256 limbs in MFMA fragment order (k_ks_gemm, fbs_kernels.hip)
    int8_t *d_ks_a = nullptr;        // scratch: digit fragments of one pass of ciphertexts
    int *d_ks_c = nullptr;           // scratch: limb sums [rows][6][cols_pad], zero between launches
    size_t ks_rows_capacity = 0;
    uint64_t *d_ks_corr = nullptr;   // [ksk_stride]  (B/2) * sum of all key-switching-key rows: balanced digits from unsigned fields
    uint64_t *d_tw_fwd = nullptr;    // [tw_table_words(N)]  psi^bitrev(i), centred doubles (layout: fbs_field.hpp)
    uint64_t *d_tw_inv = nullptr;    // [tw_table_words(N)]  psi^-bitrev(i)
    uint64_t *d_psi_pow = nullptr;    // [N] psi^x, centred doubles: what the transforms of the monomials X^e - 1 are made from (group 2)
    uint32_t *d_ms = nullptr;        // scratch: mod-switched small ciphertexts [capacity][n+1]
    size_t ms_capacity = 0;
    unsigned long long *d_ms_eps = nullptr;   // [capacity] sums of the mask words' rounding errors (zero between launches)
    uint64_t *d_ms_body = nullptr;            // [capacity] bodies before their rounding (mean-compensated modulus switch)
    uint64_t *d_acc = nullptr;       // scratch: whole accumulators [capacity][2][N] of rotations several tables share
    size_t acc_capacity = 0;         // in rows
    uint64_t *d_stage_in = nullptr, *d_stage_out = nullptr;   // device staging of the host-buffer batch call
    uint32_t *d_stage_ids = nullptr;
    size_t stage_capacity = 0;       // in ciphertexts
    uint32_t *d_idx = nullptr;       // scratch for index arrays of the host-index wires API
    size_t idx_capacity = 0;
    uint32_t *d_sk_bits = nullptr;   // [ceil(D / 32)] the GLWE secret key as packed bits (device encryption / decryption, fbs_io.hip)
    uint32_t *d_sk_lwe_bits = nullptr;   // [ceil(n / 32)] the small LWE key as packed bits (decryption of compact outputs)
    bool keys_made_on_device = false;    // the keys held now came from the device path (knob "keys_on_device"; fbs_ctx_stat)
    int64_t bsk_upload_bytes = 0;        // bootstrapping-key bytes the last key-making call copied host -> device (fbs_ctx_stat)
    uint64_t *d_compact = nullptr;   // scratch: packed compact ciphertexts of fbs_eval_seeded_compact's output groups
    size_t compact_capacity = 0;     // in words (also the staging of compact inputs, fbs_eval_sources)
    // Packed outputs (fbs_pack.hip) and folded state (fbs_fold.hip), per gadget key (parameters and bodies: HostState): the key in
    // the transform domain [rows][t][k+1][N] (centred doubles, x N^-1, key_word order), and the staging of the entry that hands
    // its result to the host (fbs_state_fetch_packed's words, fbs_state_fold's samples)
    struct GadgetKeyDev {
        double *d_key = nullptr;
        size_t capacity = 0;           // in words
        uint64_t *d_out = nullptr;
        size_t out_capacity = 0;       // in words
    } gadget_dev[2];   // [GadgetKind]
    // The scratch both share: the rounded mask fields and the raw body fields of a pass transposed to [n+1][samples N] (folding:
    // [D][samples N], then the 64-bit body words), partial accumulators [samples][slices][k+1][N]
    uint32_t *d_pack_fields = nullptr;
    size_t pack_fields_capacity = 0; // in words
    double *d_pack_acc = nullptr;
    size_t pack_acc_capacity = 0;    // in words
    // encrypted-index reads of resident state (fbs_state_lookup): the tables of a call, [tables][k+1][N], the packing scratch's
    // neighbour, grown like it; and the call's index arrays (the maps [tables][N], which table a bootstrap reads, the planes' shared source)
    uint64_t *d_lookup_tables = nullptr;
    size_t lookup_tables_capacity = 0;   // in words
    uint32_t *d_lookup_idx = nullptr;
    size_t lookup_idx_capacity = 0;      // in words
    int64_t lookup_tables = 0;           // tables the last fbs_state_lookup folded (fbs_ctx_stat)
    // encrypted tables: the accumulator bit for every bootstrap of a pass of fbs_rotate_dev (a dst_slot array, filled when it
    // grows), and the targets of an fbs_glwe_add_dev call
    uint32_t *d_acc_flags = nullptr;
    size_t acc_flags_capacity = 0;       // in words
    uint32_t *d_add_idx = nullptr;
    size_t add_idx_capacity = 0;         // in words
    // resident tables: the tables alive (fbs_ctx_destroy frees them), and the scratch of a write, grown like d_lookup_tables -- the
    // unit boxes and the turned samples, (k + 1) N words each, and the refreshed old entries of a set, D + 1 words each, a table
    std::vector<fbs_table *> tables;
    uint64_t *d_table_scratch = nullptr;
    size_t table_scratch_capacity = 0;   // in words
    uint64_t *d_pub = nullptr;       // staging of fbs_state_put_public's GLWE samples
    size_t pub_capacity = 0;         // in words
    fbs_tvset *tv_identity = nullptr;   // the identity table [0, 1, .., p - 1], made on first use: what refreshes a compact input
    int64_t *d_io_msgs = nullptr;    // scratch: messages of fbs_eval_messages, [n_inputs + n_outputs][chunk]
    size_t io_msgs_capacity = 0;     // in words
    int64_t *d_audit_err = nullptr;  // scratch of fbs_audit_level_dev: the errors [rows][s_count]
    size_t audit_err_capacity = 0;   // in words
    fbs_audit_row *d_audit_stats = nullptr;   // and the statistics [rows]
    size_t audit_stats_capacity = 0; // in rows
    uint64_t *d_wires = nullptr;     // wire slots of fbs_eval, shared by every program of the context
    size_t wires_capacity = 0;       // in words
    // The scratch buffers above are shared by every call on the context.  Calls on ONE stream are ordered by the
    // stream; a call on another stream first waits for the last user of the scratch (scratch_wait / scratch_done).
    hipStream_t scratch_stream = nullptr;
    hipEvent_t scratch_event = nullptr;
    bool scratch_used = false;

    // Resident state: the blocks fbs_state_create made and nobody destroyed yet (fbs_ctx_destroy frees them), and the link lists
    // of the current eval_sources (input links, then output links), uploaded with its first chunk
    std::vector<fbs_state *> states;
    size_t state_bytes = 0;
    fbs::WireLink *d_links = nullptr;
    size_t links_capacity = 0;
    hipEvent_t inputs_event = nullptr;   // an fbs_eval_resident that does not wait for its results: its host arrays have been read

    fbs::Profile prof;
};

// a context-owned device block of big-key ciphertexts [rows][T][D + 1]; not part of the scratch: it never moves while alive
struct fbs_state {
    fbs_ctx *ctx = nullptr;
    uint64_t *d = nullptr;
    size_t rows = 0, T = 0;
};

// context-owned folded tables [n_tab][k + 1][N] that stay where they are until freed: table (m, s) of plane m and sample s is
// number m T + s, or m where one table per plane is shared by every sample (T = 1)
struct fbs_table {
    fbs_ctx *ctx = nullptr;
    uint64_t *d = nullptr;
    uint32_t *d_unit_maps = nullptr;  // [n_tab][N]: the unit-box map of every table's writes, unit t taking ciphertext t of the write scratch
    size_t n_tab = 0, T = 0;          // T: samples a plane has tables for (1: shared)
    uint32_t n_planes = 0, len = 0, spread = 0;
    int64_t writes = 0;
};

struct fbs_tvset {
    fbs_ctx *ctx = nullptr;
    uint32_t n_tables = 0;
    uint64_t *d_tvs = nullptr;        // [n_tables + 1][N]: the tables, then TV_0 = delta_half (1 + X + .. + X^(N-1))
    uint64_t *d_post = nullptr;       // [n_tables + 1]
    std::vector<uint64_t> post;       // host copy
    // TV_F = TV_0 * D_F (host_build_tv_diff): the non-zero coefficients of the small integer polynomial D_F per table
    uint32_t diff_cap = 0;            // entries per table in the two arrays below
    uint32_t *d_diff_pos = nullptr;   // [n_tables][diff_cap]
    int32_t *d_diff_val = nullptr;    // [n_tables][diff_cap]
    uint32_t *d_diff_n = nullptr;     // [n_tables]
    std::vector<uint64_t> diff_norm2; // |D_F|^2 and |G_F|^2 (TV_F = delta_half G_F): what fusing does to the output noise
    std::vector<uint64_t> g_norm2;    //   (fbs_table_fusion_norms)
    std::vector<uint8_t> fusable;     // 0: the coefficients of D_F are too large for the 64-bit sums of k_multi_extract
};

// ---- a loaded program (fbs_program_load_ex in fbs_capi.cpp; evaluated by fbs_eval.cpp) ------------------------------------------
namespace fbs {
struct LincombStage {
    uint32_t n_out = 0;
    uint32_t *d_dst = nullptr, *d_term_off = nullptr, *d_srcs = nullptr;   // wire SLOTS
    uint64_t *d_coefs = nullptr, *d_consts = nullptr;
};
// Bootstraps of one level, sorted by source wire.  Gates that read the same wire (the reference's one-gate-one-bootstrap
// lowering emits several tables per linear combination, fbs_mapper/map_to_fbs.py:41-45, and its CSE only merges
// identical tables, fbs_mapper/fbs_exec_env.py:93-100) share one key switch + modulus switch.
struct BootStage {
    uint32_t n_gates = 0, n_sources = 0;
    uint32_t *d_src_slot = nullptr;    // [n_sources] wire slot of each distinct source
    uint32_t *d_source_of = nullptr;   // [n_gates]   index into d_src_slot
    uint32_t *d_dst = nullptr, *d_table = nullptr;   // [n_gates]
    std::vector<uint32_t> source_of;   // host copy: which key switches a slice of the level needs
    // Fused programs (FBS_LOAD_FUSE_TABLES): the tables of a source that several read are served by ONE gate of the list
    // above -- the rotation of TV_0 (table id = the set's n_tables, dst = 0x80000000 | shared index) -- and one entry each
    // of the extraction list below (k_multi_extract)
    uint32_t n_shared = 0, n_extract = 0;
    uint32_t *d_x_row = nullptr, *d_x_table = nullptr, *d_x_dst = nullptr;   // [n_extract] shared index, table, wire slot
    uint32_t *d_x_gate = nullptr;      // [n_extract] position of the shared rotation in the gate list (a level cut across GPUs
                                       // finds the accumulator in that gate's gathered row)
};
// rows of one (level, point) of the audit (fbs_audit_rows): program wire id and wire slot of each, in reporting order
struct AuditRows {
    std::vector<uint32_t> wire;
    uint32_t *d_slot = nullptr;   // [wire.size()]
};
}  // namespace fbs
struct fbs_prog {
    fbs_ctx *ctx = nullptr;
    const fbs_tvset *tv = nullptr;
    uint32_t n_inputs = 0, n_instr = 0, n_outputs = 0, n_wires = 0, n_slots = 0;
    uint32_t depth = 0, max_width = 0, max_sources = 0, n_bootstrap = 0, n_keyswitch = 0;
    uint32_t n_rotations = 0, max_shared = 0;   // blind rotations per sample (= n_bootstrap unless fused); shared rotations of the widest level
    bool fused = false;
    std::vector<uint32_t> in_slot;    // [n_inputs]
    std::vector<int64_t> out_slot;    // [n_outputs]  slot, or -1-c for the constant c
    uint32_t *d_in_slot = nullptr;    // [n_inputs]   the same on the device (fbs_eval_messages)
    uint32_t *d_out_slot = nullptr;   // [n_outputs]  slot, or 0xFFFFFFFF for a constant
    std::vector<uint32_t> live_out;   // the outputs that are wires, not constants, in output order
    uint32_t *d_live_slot = nullptr;  // [live_out.size()] their slots (the key switches of fbs_eval_seeded_compact read them)
    // schedule: for level L = 0..depth: lincomb stages (dependency order), then the bootstraps of level L+1
    std::vector<std::vector<fbs::LincombStage>> lin;   // [depth+1][sub]
    std::vector<fbs::BootStage> boot;                  // [depth]  (boot[L] = bootstraps of level L+1)
    // audited evaluation: what each point of each level reports (inputs: wire i in slot in_slot[i])
    std::vector<fbs::AuditRows> audit_lin, audit_boot;   // [depth+1], [depth]
    std::vector<std::vector<uint32_t>> audit_src;   // [depth] wire id of each distinct key-switch source
    std::vector<void *> allocations;
};
#endif   // !FBS_HOST_ONLY

namespace fbs {

// the error text of a call (fbs_error.cpp): into ctx->err, or (ctx null: fbs_ctx_create and its kin) into a thread-local that
// create_error reads
int set_error(const fbs_ctx *ctx, int code, const std::string &msg);
const char *create_error();
#define FBS_HIP(ctx, call)                                                                       \
    do {                                                                                         \
        hipError_t e__ = (call);                                                                 \
        if (e__ != hipSuccess)                                                                   \
            return fbs::set_error(ctx, FBS_E_DEVICE, std::string(#call) + ": " + hipGetErrorString(e__)); \
    } while (0)

// The ABI promises "never throws, never aborts" (include/fbs_exec.h): every extern "C" entry point is a function-try-block that
// ends in FBS_API_CATCH(owner of the error text).  translate_exception re-throws the exception in flight and maps it: an
// allocation the host cannot serve (a std::vector or std::thread sized by caller input) -> FBS_E_NOMEM, anything else ->
// FBS_E_INVALID with its what().  `report` is set_error or the searcher's equivalent; it may itself fail to allocate the text.
template <class Report>
int translate_exception(Report &&report) noexcept {
    int code = FBS_E_INVALID;
    const char *text = "unknown internal error";
    std::string what;
    try {
        throw;
    } catch (const std::bad_alloc &) {
        code = FBS_E_NOMEM, text = "out of host memory";
    } catch (const std::length_error &) {
        code = FBS_E_NOMEM, text = "out of host memory (a size computed from the arguments exceeds what a container can hold)";
    } catch (const std::exception &e) {
        try {
            what = std::string("internal error: ") + e.what();
            text = what.c_str();
        } catch (...) {
        }
    } catch (...) {
    }
    try {
        report(code, text);
    } catch (...) {
    }
    return code;
}
#define FBS_API_CATCH(owner)                                                                                          \
    catch (...) {                                                                                                     \
        const fbs_ctx *owner__ = (owner);                                                                             \
        return fbs::translate_exception([&](int code, const char *text) { fbs::set_error(owner__, code, text); });    \
    }

// host side (fbs_host.cpp)
int host_ctx_init(fbs_ctx *ctx, const fbs_params *params, uint64_t seed, const uint8_t *seed32);   // errors: text in ctx->err
void draw_secrets(fbs_ctx *ctx);   // sk_lwe, sk_glwe: the first step of host_keygen and host_keygen_seeded
void host_keygen(fbs_ctx *ctx);
void host_encrypt(const fbs_ctx *ctx, const int64_t *msgs, size_t count, uint64_t nonce0, uint64_t *cts);
void host_decrypt(const fbs_ctx *ctx, const uint64_t *cts, size_t count, int64_t *msgs);
// compact outputs (fbs_compact.hpp): words [count][compact_words(n, bits)] -> msgs[count] under sk_lwe; the device decode is held to it
void host_decrypt_compact(const fbs_ctx *ctx, const uint64_t *words, size_t count, uint32_t bits, int64_t *msgs);
// the compaction of the trivial ciphertext (0, .., 0, body): zero mask fields, the rounded body -> words[compact_words(n, bits)]
void host_compact_trivial(const fbs_ctx *ctx, uint64_t body, uint32_t bits, uint64_t *words);
// seeded path (DOM_S*): host_keygen row for row with masks under ctx->mask_key (= mask_key_of(rkey)) and noise on the seeded
// streams; the secrets are host_keygen's.  The bodies are computed, then expanded by host_expand_seeded_keys like any import.
void host_keygen_seeded(fbs_ctx *ctx);
// (mask key, bodies) -> full keys in the fbs_key_sizes layout.  bsk_bodies [G][(k+1) l][N], ksk_bodies [k N][t]
void host_expand_seeded_keys(const fbs_ctx *ctx, const RandKey &mask_key, const uint64_t *bsk_bodies, const uint64_t *ksk_bodies,
                             std::vector<uint64_t> &bsk, std::vector<uint64_t> &ksk);
// ciphertext i takes stream nonce0 + i in both DOM_SENC_MASK (under ctx->mask_key) and DOM_SENC_NOISE; bodies[count]
void host_encrypt_seeded(const fbs_ctx *ctx, const int64_t *msgs, size_t count, uint64_t nonce0, uint64_t *bodies);
// bodies[count] -> cts [count][D+1]: the mask of stream nonce0 + i under ctx->mask_key, then the body
void host_expand_seeded(const fbs_ctx *ctx, const uint64_t *bodies, size_t count, uint64_t nonce0, uint64_t *cts);
// The gadget keys (GadgetKind, above).  host_gadget_keygen -> bodies [rows][t][N]; host_expand_gadget_key: (mask key, bodies) ->
// the whole key [rows][t][k+1][N]
void host_gadget_keygen(const fbs_ctx *ctx, GadgetKind kind, uint32_t t, uint32_t gamma, std::vector<uint64_t> &bodies);
void host_expand_gadget_key(const fbs_ctx *ctx, GadgetKind kind, const RandKey &mask_key, uint32_t t, const uint64_t *bodies,
                            std::vector<uint64_t> &full);
// packed words of `count` outputs at width `bits` -> msgs[count] under sk_glwe
void host_decrypt_packed(const fbs_ctx *ctx, const uint64_t *words, size_t count, uint32_t bits, int64_t *msgs);
int host_build_tv(const fbs_ctx *ctx, const int32_t *table, uint32_t len, uint64_t *tv, uint64_t *post_add);
// the same box rule as the map of a mapped fold: what fbs_lookup_map answers (map_out [N])
int host_lookup_map(uint32_t p, uint32_t N, uint32_t len, uint32_t base, uint32_t stride, uint32_t *map_out);
// the map of a writable table, `spread` boxes an entry: what fbs_table_map answers (map_out [N]); spread = 1 is host_lookup_map
int host_table_map(uint32_t p, uint32_t N, uint32_t spread, uint32_t len, uint32_t base, uint32_t stride, uint32_t *map_out);
// D_F with TV_F = TV_0 * D_F as (position, value) pairs of its non-zero coefficients, at most p + 1 of them (`pos`, `val`
// sized for that); *norm2 = |D_F|^2, *g_norm2 = |G_F|^2 (TV_F = delta_half G_F), *abs_sum = sum |d|.  Errors as host_build_tv.
int host_build_tv_diff(const fbs_ctx *ctx, const int32_t *table, uint32_t len, uint32_t *pos, int32_t *val, uint32_t *count,
                       uint64_t *norm2, uint64_t *g_norm2, uint64_t *abs_sum);
void host_twiddles(uint32_t log_n, std::vector<uint64_t> &fwd, std::vector<uint64_t> &inv);
// public-key inputs (fbs_public.cpp): index of the first word of glwe[words] that is no canonical residue, or `words`; and the
// sample extraction glwe [ceil(count / N)][k + 1][N] -> cts [count][k N + 1] (include/fbs_exec.h, "public-key inputs", Expansion)
size_t first_noncanonical(const uint64_t *w, size_t words);
void host_pub_expand(uint32_t k, uint32_t N, const uint64_t *glwe, size_t count, uint64_t *cts);
// fbs_import_keys: null if sampled rows of bsk and ksk decrypt under sk_lwe [n] and sk_glwe [D] as the fbs_key_sizes layout says,
// else why not
const char *imported_keys_mismatch(const fbs_ctx *ctx, const uint64_t *sk_lwe, const uint64_t *sk_glwe, const uint64_t *bsk,
                                   const uint64_t *ksk);

#ifndef FBS_HOST_ONLY
// device side (fbs_kernels.hip); all asynchronous on `stream`
int dev_upload_keys(fbs_ctx *ctx);       // BSK -> NTT domain, KSK padded: the three below, from the host copies
int dev_upload_tables(fbs_ctx *ctx);     // twiddle tables; allocates the device buffers of the keys on first use
int dev_upload_ksk(fbs_ctx *ctx);        // ctx->ksk -> d_ksk (padded), d_ksk_f, d_ks_corr, the GEMM's fragments
// the bootstrapping key, coefficient domain -> d_bsk_hat (and d_bsk_hat_small): from d_src on the device, or (null) from ctx->bsk,
// which is then uploaded and counted in bsk_upload_bytes; blocks until the transforms are done
int dev_transform_bsk(fbs_ctx *ctx, const uint64_t *d_src);
// Keys on the device (fbs_keygen.hip; knob "keys_on_device"), word for word the host functions.  dev_make_keys: after the secrets
// and the tables are on the device, both evaluation keys made there (seeded: host_keygen_seeded under `mask_key`, else host_keygen)
// or, bsk_bodies / ksk_bodies (host arrays) non-null, expanded there (host_expand_seeded_keys under `mask_key`; no secret); the
// bootstrapping key transformed from the device rows, and ctx->bsk / ctx->ksk filled from them.  dev_gadget_bodies:
// host_gadget_keygen's bodies [rows][t][N]
int dev_make_keys(fbs_ctx *ctx, bool seeded, const RandKey &mask_key, const uint64_t *bsk_bodies, const uint64_t *ksk_bodies);
int dev_gadget_bodies(fbs_ctx *ctx, GadgetKind kind, uint32_t t, uint32_t gamma, std::vector<uint64_t> &bodies);
int dev_keyswitch_gemm_setup(fbs_ctx *ctx);   // limb fragments of the key-switching key for the int8 MFMA key switch
// the key switch kN -> n and the rounding of every word to Z_(2^log2_mod) (log2(2N): what the blind rotation reads; up to 31: the
// fields of compact outputs), into d_ms [gv.ks_count][n + 1]
int dev_keyswitch(fbs_ctx *ctx, const GateView &gv, uint32_t *d_ms, uint32_t log2_mod, hipStream_t stream);
int dev_keyswitch_reserve(fbs_ctx *ctx, size_t count);          // scratch of the GEMM key switch for launches of `count` (blocks when it grows)
int dev_keyswitch_rezero(fbs_ctx *ctx, hipStream_t stream);     // puts its "zero between launches" scratch back after a failed call
// `start` (encrypted-index reads): the GLWE samples the rotations start from instead of the trivial sample of a table -- `tv` may
// then be null, no constant is added at the extraction, and the fused path (accumulator rows) is refused
struct BrStart {
    const uint64_t *d_acc0;     // [n_acc][(k + 1) N] canonical residues, 16-byte aligned
    uint32_t n_acc;
    const uint32_t *d_acc_of;   // [first + gv.count] device memory, or null: bootstrap i starts from sample first + i
    size_t first;               // the pass's first bootstrap, counted within the entry's call (an entry may run in passes)
    // encrypted tables (fbs_rotate_dev): the rotated sample itself is wanted, not an entry of it -- the view names out_rows of
    // (k + 1) N words and a dst_slot whose entries carry the accumulator bit, and every bootstrap leaves its whole accumulator there
    bool whole = false;
};
int dev_blind_rotate(fbs_ctx *ctx, const fbs_tvset *tv, const GateView &gv, const uint32_t *d_ms, hipStream_t stream,
                     const BrStart *start = nullptr);
// `T` = sample stride of the wire buffer, samples [s_begin, s_begin + s_count) are computed
int dev_lincomb(fbs_ctx *ctx, uint64_t *d_wires, size_t T, size_t s_begin, size_t s_count, uint32_t n_out,
                const uint32_t *d_dst, const uint32_t *d_term_off, const uint32_t *d_srcs, const uint64_t *d_coefs,
                const uint64_t *d_consts, hipStream_t stream);
// rows[f - f_begin] -> wire slot dst_slot[f / s_count], sample s_begin + f % s_count, for f in [f_begin, f_begin + count)
// (row_words = 0: rows are ciphertexts; else the row stride, and gates whose dst_slot has bit 31 set -- shared rotations -- are skipped)
int dev_scatter_rows(fbs_ctx *ctx, uint64_t *d_wires, size_t T, size_t s_begin, size_t s_count, const uint32_t *d_dst_slot,
                     const uint64_t *d_rows, size_t f_begin, size_t count, uint32_t row_words, hipStream_t stream);
// rows of `count` ciphertexts: out[i] = wires[slot][s_begin + i] (slot >= 0) or the trivial ciphertext of `body`
int dev_copy_out(fbs_ctx *ctx, const uint64_t *d_wires, size_t T, size_t s_begin, size_t count, int64_t slot, uint64_t body,
                 uint64_t *d_out, hipStream_t stream);
// out[slot x_dst[e]][s] = SampleExtract_0(acc_rows[x_row[e] * s_count + s - s_begin] * D_table) + post, for the n_extract
// tables e that share rotations of TV_0, samples [s_begin, s_begin + s_count)
int dev_multi_extract(fbs_ctx *ctx, const fbs_tvset *tv, const uint64_t *d_acc_rows, uint64_t *d_wires, size_t T, size_t s_begin,
                      size_t s_count, uint32_t n_extract, const uint32_t *d_x_row, const uint32_t *d_x_table,
                      const uint32_t *d_x_dst, hipStream_t stream);
int dev_polymul(fbs_ctx *ctx, const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_c, hipStream_t stream);
// test hooks (fbs_debug_transform.hip): host arrays in and out, synchronous
int dev_debug_field(fbs_ctx *ctx, int op, const int64_t *x, const int64_t *w, size_t count, int64_t *out);
const char *debug_transform_list();
int dev_debug_transform(fbs_ctx *ctx, const char *variant, const int64_t *in, int64_t *out, size_t polys);
// gauss_sample (fbs_sampler.hpp) of the windows d_words [count][6] -> d_out [count], one thread each (fbs_io.hip); asynchronous on `stream`
int dev_debug_gauss(const fbs_ctx *ctx, const uint64_t *d_words, size_t count, uint64_t sigma, int64_t *d_out, hipStream_t stream);

// device encryption / decryption under the big key (fbs_io.hip), word for word host_encrypt / host_decrypt; asynchronous on `stream`
int dev_upload_secret(fbs_ctx *ctx);     // sk_glwe -> d_sk_bits (after keygen or import)
// ciphertext (r, s) of `v` takes stream nonce0 + r * nonce_stride + s
int dev_encrypt(const fbs_ctx *ctx, const IoView &v, uint64_t nonce0, uint64_t nonce_stride, hipStream_t stream);
int dev_decrypt(const fbs_ctx *ctx, const IoView &v, hipStream_t stream);
// seeded path, word for word host_encrypt_seeded / host_expand_seeded.  dev_encrypt_seeded: d_msgs [count] -> d_bodies [count];
// dev_expand_seeded: the bodies at v.msgs (read as uint64 words) -> ciphertexts, (r, s) on stream nonce0 + r nonce_stride + s
int dev_encrypt_seeded(const fbs_ctx *ctx, const int64_t *d_msgs, size_t count, uint64_t nonce0, uint64_t *d_bodies, hipStream_t stream);
int dev_expand_seeded(const fbs_ctx *ctx, const IoView &v, uint64_t nonce0, uint64_t nonce_stride, hipStream_t stream);

// compact outputs (fbs_compact.hip): the switched fields d_ms [count][n + 1] -> packed words d_words [count][W]; and the decode of
// packed words under the small key (d_sk_lwe_bits), word for word host_decrypt_compact
int dev_compact_pack(const fbs_ctx *ctx, const uint32_t *d_ms, size_t count, uint32_t bits, uint64_t *d_words, hipStream_t stream);
int dev_decrypt_compact(const fbs_ctx *ctx, const uint64_t *d_words, size_t count, uint32_t bits, int64_t *d_msgs, hipStream_t stream);
// and back: packed words [count][W] at width `bits` -> the fields at log2(2N) bits, d_ms [count][n + 1] as the blind rotation reads them
// (re-rounded as the modulus switch rounds when bits > log2(2N))
int dev_compact_unpack(const fbs_ctx *ctx, const uint64_t *d_words, size_t count, uint32_t bits, uint32_t *d_ms, hipStream_t stream);

// packed outputs (fbs_pack.hip).  dev_upload_gadget_key: the whole key of `kind` in the coefficient domain -> its d_key
// (transformed on the device; blocks).  pack_slices_for: slices
// per sample of a launch of `samples` samples whose sum runs over `rows` key rows (n for packing, D for folding).  dev_pack: the
// switched 31-bit fields d_ms [count][n + 1] of ciphertexts that start a packed sample -> packed words at width `bits`; uses
// d_pack_fields ((n + 1) * samples * N words) and d_pack_acc (samples * slices * (k + 1) * N words), which the caller has sized
int dev_upload_gadget_key(fbs_ctx *ctx, GadgetKind kind, const std::vector<uint64_t> &full, uint32_t t);
uint32_t pack_slices_for(const fbs_ctx *ctx, size_t samples, uint32_t rows);
int dev_pack(fbs_ctx *ctx, const uint32_t *d_ms, size_t count, uint32_t bits, uint64_t *d_words, hipStream_t stream);
// k_pack_accumulate alone, on the fields, key and row count of `a` (fbs_pack.hpp): samples * a.slices workgroups
struct PackArgs;
int dev_pack_accumulate(const fbs_ctx *ctx, const PackArgs &a, size_t samples, hipStream_t stream);
// folded state (fbs_fold.hip).  dev_fold: the big-key ciphertexts d_cts [count][D + 1] that start a folded sample -> the samples
// d_glwe [ceil(count / N)][k + 1][N]; uses d_pack_fields (D * samples * N + 2 * samples * N words) and d_pack_acc, which the caller
// has sized.  dev_fold_front: its first kernel alone, d_cts -> d_fields [D][cols] rounded to tg bits, then cols body words.
// d_map (the mapped fold, "encrypted-index reads" in include/fbs_exec.h): position j takes ciphertext d_map[j] of the n_src at d_cts
int dev_fold(fbs_ctx *ctx, const uint64_t *d_cts, size_t count, uint64_t *d_glwe, hipStream_t stream, const uint32_t *d_map = nullptr,
             size_t n_src = 0);
int dev_fold_front(const fbs_ctx *ctx, const uint64_t *d_cts, size_t count, uint32_t cols, uint32_t tg, uint32_t *d_fields, hipStream_t stream);

// encrypted tables (fbs_table.hip).  dev_ms_negate: every amount of `rows` modulus-switched rows [n + 1] -> (2N - a) mod 2N.
// dev_glwe_add: sample d_dst_of[f] of d_dst += sample f of d_src mod q, f < count, (k + 1) N words a sample; d_dst_of (device) holds
// what the host checked: targets in range, none twice
int dev_ms_negate(const fbs_ctx *ctx, uint32_t *d_ms, size_t rows, hipStream_t stream);
int dev_glwe_add(const fbs_ctx *ctx, uint64_t *d_dst, const uint64_t *d_src, const uint32_t *d_dst_of, size_t count, hipStream_t stream);
// dev_ct_sub: ciphertext f of d_out = ciphertext d_a_of[f] of d_a - ciphertext f of d_b mod q, f < count, D + 1 words each (d_out may
// be d_b; d_b null: nothing is taken off, a gather); d_a_of (device) holds what the host checked
int dev_ct_sub(const fbs_ctx *ctx, const uint64_t *d_a, const uint32_t *d_a_of, const uint64_t *d_b, uint64_t *d_out, size_t count, hipStream_t stream);

// audited evaluation (fbs_audit.hip): errors of the big-key ciphertexts in slots d_row_slot[rows], samples [s_begin, s_begin + s_count),
// against d_expected [rows][s_count] -> d_err [rows][s_count] (wire units); of the switched fields d_ms [rows * s_count][n + 1] at
// log2(2N) bits (field units); and the exact statistics of each row of d_err -> d_stats [rows].  One call takes at most
// AUDIT_MAX_SAMPLES samples a row: below that neither the 64-bit sum nor the 128-bit sum of squares can overflow
constexpr size_t AUDIT_MAX_SAMPLES = (size_t)1 << 18;
int dev_audit_wire(const fbs_ctx *ctx, const uint64_t *d_wires, const uint32_t *d_row_slot, size_t rows, size_t T, size_t s_begin,
                   size_t s_count, const int64_t *d_expected, int64_t *d_err, hipStream_t stream);
int dev_audit_fields(const fbs_ctx *ctx, const uint32_t *d_ms, size_t rows, size_t s_count, const int64_t *d_expected, int64_t *d_err,
                     hipStream_t stream);
int dev_audit_reduce(const fbs_ctx *ctx, const int64_t *d_err, size_t rows, size_t s_count, bool fields, fbs_audit_row *d_stats,
                     hipStream_t stream);

// the device-side inputs and outputs of a chunk (fbs_state.hip): the links of `a` into their wire slots, or out of them into state
// rows, one launch each; the group sums of `a`, one launch
int dev_wire_load(const fbs_ctx *ctx, const WireCopy &a, hipStream_t stream);
int dev_wire_store(const fbs_ctx *ctx, const WireCopy &a, hipStream_t stream);
int dev_state_sum_groups(const fbs_ctx *ctx, const SumGroups &a, hipStream_t stream);
// public-key inputs (fbs_public.hip): sample extraction of the GLWE samples d_glwe [ceil(count / N)][k + 1][N] into the big-key
// ciphertexts d_cts [count][D + 1], message j from coefficient j mod N of sample j / N; word for word host_pub_expand
int dev_expand_public(const fbs_ctx *ctx, const uint64_t *d_glwe, size_t count, uint64_t *d_cts, hipStream_t stream);

// ---- host side of the device library: what the entries of fbs_capi.cpp and fbs_eval.cpp share (defined in fbs_capi.cpp) --------
hipStream_t pick(const fbs_ctx *ctx, void *stream);   // the caller's stream, or the context's
// what an entry on a loaded program checks first: the keys, the device, the program's owner
int check_prog(fbs_ctx *ctx, const fbs_prog *prog);
int sync_stream(fbs_ctx *ctx, hipStream_t s);
bool state_of(const fbs_ctx *ctx, const fbs_state *st);   // a live state of this context
// Scratch is grown on demand, and growing it BLOCKS.  One scratch buffer of `count` elements of `bytes` each; `counted`: a growth
// shows in scratch_growths
template <typename T>
int grow(fbs_ctx *ctx, T *&buf, size_t &capacity, size_t count, size_t bytes, bool counted) {
    if (count <= capacity) return FBS_OK;
    if (counted) ctx->scratch_growths++;
    if (ctx->scratch_used) FBS_HIP(ctx, hipStreamSynchronize(ctx->scratch_stream));   // kernels may still read the old buffer
    if (buf) (void)hipFree(buf);
    buf = nullptr;
    capacity = 0;
    FBS_HIP(ctx, hipMalloc(&buf, count * bytes));
    capacity = count;
    return FBS_OK;
}
int ensure_ms(fbs_ctx *ctx, size_t count);       // modulus-switch scratch (and the GEMM key switch's) for `count` ciphertexts
int ensure_acc(fbs_ctx *ctx, size_t rows);       // whole accumulators
int ensure_wires(fbs_ctx *ctx, size_t words);
int ensure_io_msgs(fbs_ctx *ctx, size_t words);
int ensure_idx(fbs_ctx *ctx, size_t words);
int identity_tv(fbs_ctx *ctx, fbs_tvset **out);  // the context's identity table, made on first use
// cross-stream ordering of the scratch: wait before the first use, done after the last, fail (which returns rc) on an error between
int scratch_wait(fbs_ctx *ctx, hipStream_t s);
int scratch_done(fbs_ctx *ctx, hipStream_t s);
int scratch_fail(fbs_ctx *ctx, hipStream_t s, int rc);
// launch views: the plain batch (gate g = ciphertext g), and `ng` wire slots d_slot (device) of a chunk of tc samples, stride Tc
GateView batch_view(const uint64_t *in, uint64_t *out, const uint32_t *table_ids, size_t count);
GateView slots_view(const uint64_t *in, uint64_t *out, const uint32_t *d_slot, size_t ng, size_t Tc, size_t tc);
// `count` ciphertexts through the modulus-switch scratch, in passes of what the context has of it or of this many when it has less,
// under scratch_wait / scratch_fail / scratch_done: `pass(f0, rows)` queues ciphertexts [f0, f0 + rows) on `s`
constexpr size_t COMPACT_PASS = 8192;
size_t ms_pass_size(const fbs_ctx *ctx, size_t count);
int ms_passes(fbs_ctx *ctx, size_t count, hipStream_t s, const std::function<int(size_t f0, size_t rows)> &pass);

// profiling helpers
void prof_begin(fbs_ctx *ctx, int which, hipStream_t s, hipEvent_t *e0, hipEvent_t *e1);
void prof_end(fbs_ctx *ctx, int which, hipStream_t s, hipEvent_t e0, hipEvent_t e1);
#endif   // !FBS_HOST_ONLY

}  // namespace fbs

// The client's entries of include/fbs_exec.h that never turn to a device -- sizes, exports, encryption, decryption and seeded
// expansion on host buffers, the decoders of compact and packed outputs, the error text -- written once for both libraries that
// serve them: compiled into libfbsexec.so and, with FBS_HOST_ONLY, into libfbsclient.so, as fbs_public.cpp is for its entries.
// Host code with no device in it: it reads and writes the host state of a context (fbs::HostState) and nothing else, which the
// host-only build enforces.  The entries that differ between the libraries (contexts, key generation) are fbs_capi.cpp's and
// fbs_client_capi.cpp's; what those share is in fbs_api_checks.hpp.
#include <cstring>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "fbs_api_checks.hpp"
#include "fbs_compact.hpp"
#include "fbs_internal.hpp"
#include "fbs_pack.hpp"

using namespace fbs;

extern "C" {

// ---------------------------------------------------------------------------------------------
int fbs_poly_size_check(uint32_t poly_size) try {
    if (poly_size == 0) return set_error(nullptr, FBS_E_INVALID, "polynomial size 0");
    if (poly_size & (poly_size - 1)) {
        uint32_t pow2 = poly_size & (~poly_size + 1);   // largest power of two dividing N
        return set_error(nullptr, FBS_E_POLY_SIZE,
                         "N = " + std::to_string(poly_size) + " is not a power of two: X^N + 1 then has the factor X^" +
                             std::to_string(pow2) + " + 1, so a GLWE sample over it is no harder than one of degree " +
                             std::to_string(pow2) + "; use a power-of-two N (256 .. 4096) and any plaintext modulus p");
    }
    if (poly_size < 256 || poly_size > 4096)
        return set_error(nullptr, FBS_E_INVALID, "supported polynomial sizes are N = 256, 512, 1024, 2048, 4096");
    return FBS_OK;
} FBS_API_CATCH(nullptr)

int fbs_ctx_create_seeded(const fbs_params *params, const uint8_t seed[32], int device, fbs_ctx **out) try {
    if (!seed) return set_error(nullptr, FBS_E_INVALID, "null seed");
    return ctx_create(params, 0, seed, device, out);
} FBS_API_CATCH(nullptr)

const char *fbs_last_error(const fbs_ctx *ctx) { return ctx ? ctx->err.c_str() : create_error(); }

// ---------------------------------------------------------------------------------------------
int fbs_key_sizes(const fbs_ctx *ctx, size_t sizes[4]) try {
    if (!ctx || !sizes) return FBS_E_INVALID;
    sizes[0] = ctx->p.n;
    sizes[1] = ctx->D;
    sizes[2] = ctx->n_ggsw * ctx->rows * (ctx->p.k + 1) * ctx->N;
    sizes[3] = (size_t)ctx->D * ctx->p.t_ksk * (ctx->p.n + 1);
    return FBS_OK;
} FBS_API_CATCH(ctx)

int fbs_export_keys(const fbs_ctx *ctx, uint64_t *sk_lwe, uint64_t *sk_glwe, uint64_t *bsk, uint64_t *ksk) try {
    if (!ctx) return FBS_E_INVALID;
    if (!ctx->have_keys) return set_error(ctx, FBS_E_STATE, "fbs_keygen has not run");
    if ((sk_lwe || sk_glwe) && ctx->eval_only) return set_error(ctx, FBS_E_STATE, EVAL_ONLY);
    if (sk_lwe) std::memcpy(sk_lwe, ctx->sk_lwe.data(), ctx->sk_lwe.size() * 8);
    if (sk_glwe) std::memcpy(sk_glwe, ctx->sk_glwe.data(), ctx->sk_glwe.size() * 8);
    if (bsk) std::memcpy(bsk, ctx->bsk.data(), ctx->bsk.size() * 8);
    if (ksk) std::memcpy(ksk, ctx->ksk.data(), ctx->ksk.size() * 8);
    return FBS_OK;
} FBS_API_CATCH(ctx)

// ---- encrypt / decrypt under the big key -----------------------------------------------------
int fbs_encrypt_fresh(fbs_ctx *ctx, const int64_t *msgs, size_t count, uint64_t *cts, uint64_t *nonce0) try {
    uint64_t first = 0;
    if (int rc = io_prologue(ctx, msgs, cts, count, IO_SECRET | IO_FRESH, &first)) return rc;
    if (nonce0) *nonce0 = first;
    host_encrypt(ctx, msgs, count, first, cts);
    return FBS_OK;
} FBS_API_CATCH(ctx)

int fbs_encrypt(const fbs_ctx *ctx, const int64_t *msgs, size_t count, uint64_t nonce0, uint64_t *cts) try {
    if (int rc = io_prologue(ctx, msgs, cts, count, IO_SECRET | IO_BELOW_2_55, &nonce0)) return rc;
    host_encrypt(ctx, msgs, count, nonce0, cts);
    return FBS_OK;
} FBS_API_CATCH(ctx)

int fbs_decrypt(const fbs_ctx *ctx, const uint64_t *cts, size_t count, int64_t *msgs) try {
    if (int rc = io_prologue(ctx, cts, msgs, count, IO_SECRET, nullptr)) return rc;
    host_decrypt(ctx, cts, count, msgs);
    return FBS_OK;
} FBS_API_CATCH(ctx)

// ---- seeded keys and inputs: masks under a public key, only bodies travel ----------------------
int fbs_seeded_key_sizes(const fbs_ctx *ctx, size_t sizes[2]) try {
    if (!ctx || !sizes) return FBS_E_INVALID;
    sizes[0] = ctx->n_ggsw * ctx->rows * ctx->N;
    sizes[1] = (size_t)ctx->D * ctx->p.t_ksk;
    return FBS_OK;
} FBS_API_CATCH(ctx)

int fbs_export_seeded_keys(const fbs_ctx *ctx, uint8_t mask_key[32], uint64_t *bsk_bodies, uint64_t *ksk_bodies) try {
    if (!ctx) return FBS_E_INVALID;
    if (!mask_key || !bsk_bodies || !ksk_bodies) return set_error(ctx, FBS_E_INVALID, "null argument");
    if (!ctx->have_keys) return set_error(ctx, FBS_E_STATE, "fbs_keygen has not run");
    if (ctx->eval_only) return set_error(ctx, FBS_E_STATE, EVAL_ONLY);
    if (!ctx->seeded_keys) return set_error(ctx, FBS_E_STATE, "the keys of this context did not come from fbs_keygen_seeded");
    const uint32_t N = ctx->N, n = ctx->p.n, k = ctx->p.k;
    const size_t bsk_rows = ctx->n_ggsw * ctx->rows, ksk_rows = (size_t)ctx->D * ctx->p.t_ksk;
    for (int i = 0; i < 8; i++)
        for (int b = 0; b < 4; b++) mask_key[4 * i + b] = (uint8_t)(ctx->mask_key.w[i] >> (8 * b));
    for (size_t r = 0; r < bsk_rows; r++)
        std::memcpy(bsk_bodies + r * N, ctx->bsk.data() + (r * (k + 1) + k) * (size_t)N, (size_t)N * 8);
    for (size_t r = 0; r < ksk_rows; r++) ksk_bodies[r] = ctx->ksk[r * (n + 1) + n];
    return FBS_OK;
} FBS_API_CATCH(ctx)

int fbs_encrypt_seeded(const fbs_ctx *ctx, const int64_t *msgs, size_t count, uint64_t nonce0, uint64_t *bodies) try {
    if (int rc = io_prologue(ctx, msgs, bodies, count, IO_SECRET | IO_BELOW_2_55, &nonce0)) return rc;
    host_encrypt_seeded(ctx, msgs, count, nonce0, bodies);
    return FBS_OK;
} FBS_API_CATCH(ctx)

int fbs_encrypt_seeded_fresh(fbs_ctx *ctx, const int64_t *msgs, size_t count, uint64_t *bodies, uint64_t *nonce0) try {
    uint64_t first = 0;
    if (int rc = io_prologue(ctx, msgs, bodies, count, IO_SECRET | IO_FRESH, &first)) return rc;
    if (nonce0) *nonce0 = first;
    host_encrypt_seeded(ctx, msgs, count, first, bodies);
    return FBS_OK;
} FBS_API_CATCH(ctx)

// (no secret needed: runs on evaluation-only contexts)
int fbs_expand_seeded(const fbs_ctx *ctx, const uint64_t *bodies, size_t count, uint64_t nonce0, uint64_t *cts) try {
    if (int rc = io_prologue(ctx, bodies, cts, count, IO_BELOW_2_56 | IO_CT_WORDS, &nonce0)) return rc;
    host_expand_seeded(ctx, bodies, count, nonce0, cts);
    return FBS_OK;
} FBS_API_CATCH(ctx)

// ---- compact outputs: the decoder (fbs_compact.hpp) --------------------------------------------
int fbs_compact_words(const fbs_ctx *ctx, uint32_t bits, size_t *words) try {
    if (!ctx || !words) return FBS_E_INVALID;
    if (int rc = check_bits(ctx, bits)) return rc;
    *words = compact_words(ctx->p.n, bits);
    return FBS_OK;
} FBS_API_CATCH(ctx)

int fbs_decrypt_compact(const fbs_ctx *ctx, const uint64_t *words, size_t count, uint32_t bits, int64_t *msgs) try {
    if (int rc = io_prologue(ctx, words, msgs, count, IO_SECRET, nullptr)) return rc;
    if (int rc = check_bits(ctx, bits)) return rc;
    if (int rc = check_compact_words(ctx, count, bits)) return rc;
    host_decrypt_compact(ctx, words, count, bits, msgs);
    return FBS_OK;
} FBS_API_CATCH(ctx)

// ---- packed outputs: the packing key's sizes and export, the decoder (fbs_pack.hpp) ------------
int fbs_packing_key_sizes(const fbs_ctx *ctx, uint32_t t_p, size_t sizes[2]) try {
    return gadget_key_sizes(ctx, GK_PACK, t_p, sizes);
} FBS_API_CATCH(ctx)

int fbs_export_packing_key(const fbs_ctx *ctx, uint64_t *bodies, uint64_t *full) try {
    return gadget_key_export(ctx, GK_PACK, bodies, full);
} FBS_API_CATCH(ctx)

int fbs_packed_words(const fbs_ctx *ctx, size_t count, uint32_t bits, size_t *words) try {
    if (!ctx || !words) return FBS_E_INVALID;
    if (int rc = check_bits(ctx, bits)) return rc;
    if (int rc = check_packed_words(ctx, count, bits)) return rc;
    *words = packed_words(ctx->p.k, ctx->N, count, bits);
    return FBS_OK;
} FBS_API_CATCH(ctx)

int fbs_decrypt_packed(const fbs_ctx *ctx, const uint64_t *words, size_t count, uint32_t bits, int64_t *msgs) try {
    if (int rc = io_prologue(ctx, words, msgs, count, IO_SECRET, nullptr)) return rc;
    if (int rc = check_bits(ctx, bits)) return rc;
    if (int rc = check_packed_words(ctx, count, bits)) return rc;
    host_decrypt_packed(ctx, words, count, bits, msgs);
    return FBS_OK;
} FBS_API_CATCH(ctx)

// test hook: raise inside an entry point what a host allocation or a library call could raise, to show the barrier holds
// (kind 0: std::bad_alloc, 1: std::length_error, 2: std::runtime_error, 3: a non-standard exception; anything else: no throw)
int fbs_debug_raise(fbs_ctx *ctx, int kind) try {
    if (kind == 0) throw std::bad_alloc();
    if (kind == 1) throw std::length_error("vector::_M_default_append");
    if (kind == 2) throw std::runtime_error("raised on request");
    if (kind == 3) throw 42;
    return FBS_OK;
} FBS_API_CATCH(ctx)

}  // extern "C"

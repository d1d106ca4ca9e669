// What the entries of include/fbs_exec.h that run on the host check before they do anything -- buffers, keys, the secret, the
// stream ranges, word counts that must not overflow, the fresh-stream counter, the widths of compact and packed outputs, the
// packing key's parameters -- in one place, because two libraries serve those entries: libfbsexec.so and the client library
// libfbsclient.so.  The entries that never turn to a device are one text compiled into both (fbs_client_entries.cpp); those that
// differ -- contexts, key generation -- are fbs_capi.cpp's and fbs_client_capi.cpp's, and what the two share of them (parameter
// admission, the common statistics, the state changes of a key generation) is here as well.  The same checks in the same order
// give the same codes and texts, and a refused call moves no counter in either.  The public-key entries (fbs_public.cpp:
// libfbsexec.so and libfbspublic.so) take their parameter admission from here.  Host code, no device in it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <memory>
#include <string>

#include "fbs_compact.hpp"
#include "fbs_internal.hpp"
#include "fbs_pack.hpp"

namespace fbs {

// what every entry that needs the secret keys says on a context made by fbs_import_seeded_keys
constexpr const char *EVAL_ONLY = "this context holds evaluation keys only";

// Parameter admission, what fbs_ctx_create applies in either library: the range rules of host_ctx_init (everything that is
// arithmetic on the set: derived sizes, Delta, gadget factors, the random key from `seed` or `seed32`), then whether a kernel is
// built for the set -- keys for a set no server can evaluate are of no use -- with the codes and texts left as the thread's
// creation error.  *out: a context for the set with its host state filled in, the caller's to delete.
// static: it allocates an fbs_ctx, whose size is the library's own (the host state alone under FBS_HOST_ONLY, the device side too
// in libfbsexec.so).  An exported inline copy could be taken from another library loaded into the same process -- libfbsexec.so
// is not linked -Bsymbolic -- and hand the GPU library a context too small for what it writes.  No library exports these two.
static inline int admit_params(const fbs_params *params, uint64_t seed, const uint8_t *seed32, fbs_ctx **out) {
    if (!params) return set_error(nullptr, FBS_E_INVALID, "null argument");
    std::unique_ptr<fbs_ctx> ctx(new fbs_ctx);
    int rc = host_ctx_init(ctx.get(), params, seed, seed32);
    if (rc == FBS_OK)
        if (const char *why = kernel_not_built(ctx->p)) rc = set_error(ctx.get(), FBS_E_INVALID, why);
    if (rc != FBS_OK) return set_error(nullptr, rc, ctx->err);
    *out = ctx.release();
    return FBS_OK;
}
// ... for the entries that take a parameter set and no context (fbs_pub_*): *probe tells them N, D and Delta
static inline int params_admitted(const fbs_params *params, fbs_ctx **probe) { return admit_params(params, 0, nullptr, probe); }

// fbs_ctx_create and fbs_ctx_create_seeded (fbs_client_entries.cpp) of a library end here: admit_params, then that library's rule
// for `device`.  Each library has its own (fbs_capi.cpp, fbs_client_capi.cpp; libfbspublic.so has none and calls none); hidden,
// so that a process that has loaded both never takes one library's for the other's.  Declared here, once, so that the two
// definitions and the caller are checked against one signature.
__attribute__((visibility("hidden"))) int ctx_create(const fbs_params *params, uint64_t seed, const uint8_t *seed32, int device, fbs_ctx **out);

// a message about a gadget key: '@' stands for the kind's noun ("packing", "fold"), '#' for the letter of its parameters (t_p, t_f)
inline std::string gadget_text(GadgetKind kind, const std::string &pattern) {
    std::string text;
    for (char c : pattern) {
        if (c == '@') text += GADGET_KINDS[kind].noun;
        else if (c == '#') text += GADGET_KINDS[kind].letter;
        else text += c;
    }
    return text;
}
// the three statistics of a gadget key: <noun>_key, <noun>_levels, <noun>_base_bits; false: `k` is none of them
inline bool gadget_stat(const fbs_ctx *ctx, GadgetKind kind, const std::string &k, int64_t *value) {
    const HostState::GadgetKeyState &key = ctx->gadget[kind];
    if (k == gadget_text(kind, "@_key")) *value = key.have;
    else if (k == gadget_text(kind, "@_levels")) *value = key.have ? key.t : 0;
    else if (k == gadget_text(kind, "@_base_bits")) *value = key.have ? key.gamma : 0;
    else return false;
    return true;
}

// The statistics of fbs_ctx_stat that both libraries answer; false: not one of them (the GPU library goes on to its own)
inline bool host_stat(const fbs_ctx *ctx, const std::string &k, int64_t *value) {
    if (k == "next_nonce") *value = (int64_t)ctx->next_nonce.load();
    else if (k == "has_secret") *value = ctx->have_keys && !ctx->eval_only;
    else if (k == "seeded_keys") *value = ctx->have_keys && ctx->seeded_keys;
    else return gadget_stat(ctx, GK_PACK, k, value);
    return true;
}

// What a call that replaces the keys of a context does to its state: which kind the new keys are, as soon as the host has them;
// and, once they are in place (in the GPU library: on the device), that there are keys -- and no packing key any more
inline void keys_replaced(fbs_ctx *ctx, bool seeded, bool eval_only) {
    ctx->seeded_keys = seeded;
    ctx->eval_only = eval_only;
}
inline void keys_in_place(fbs_ctx *ctx) {
    ctx->have_keys = true;
    for (auto &key : ctx->gadget) key.have = false;   // (a packing key, a fold key belonged to the keys this call replaced)
}

// Streams [first, first + count) of [2^55, 2^56) that nobody has used, for every entry that takes fresh streams.  The range is
// reserved atomically: two threads encrypting on one context never share a stream (the bound is checked BEFORE the counter
// moves, so a refused call leaves it where it was).
inline int reserve_fresh(const fbs_ctx *ctx, size_t count, uint64_t *first_out) {
    uint64_t first = ctx->next_nonce.load(std::memory_order_relaxed);
    do {
        if (count > (1ull << 56) || first + count > (1ull << 56)) return set_error(ctx, FBS_E_STATE, "encryption streams of this context are used up");
    } while (!ctx->next_nonce.compare_exchange_weak(first, first + count, std::memory_order_relaxed));
    *first_out = first;
    return FBS_OK;
}
// streams [2^55, 2^56) belong to the fresh entries: an explicit nonce can never repeat one the context handed out itself
inline int check_nonces(const fbs_ctx *ctx, uint64_t nonce0, size_t count) {
    if (nonce0 >= (1ull << 55) || count > (1ull << 55) - nonce0) return set_error(ctx, FBS_E_INVALID, "nonce0 + count must stay below 2^55");
    return FBS_OK;
}
// seeded streams may be any the full entries may take, fresh ones included
inline int check_seeded_streams(const fbs_ctx *ctx, uint64_t nonce0, size_t count) {
    if (nonce0 >= (1ull << 56) || count > (1ull << 56) - nonce0) return set_error(ctx, FBS_E_INVALID, "nonce0 + count must stay below 2^56");
    return FBS_OK;
}
// count ciphertexts of D + 1 words: more than fit in a size_t is refused before anything is launched
inline int check_ct_words(const fbs_ctx *ctx, size_t count) {
    if (count > SIZE_MAX / 8 / (ctx->D + 1)) return set_error(ctx, FBS_E_INVALID, "count * (D + 1) words overflow");
    return FBS_OK;
}

// What the encrypt / decrypt / expand entries check, in this order: the buffers (a null one with count > 0 is FBS_E_INVALID
// without a message), the keys, the secret (IO_SECRET), the explicit streams [*first, *first + count) (IO_BELOW_2_55 or
// IO_BELOW_2_56), count * (D + 1) words (IO_CT_WORDS), and last a fresh range (IO_FRESH: reserved into *first), so that a
// refused call never moves next_nonce.
enum : unsigned { IO_SECRET = 1, IO_BELOW_2_55 = 2, IO_BELOW_2_56 = 4, IO_FRESH = 8, IO_CT_WORDS = 16 };
inline int io_prologue(const fbs_ctx *ctx, const void *src, const void *dst, size_t count, unsigned checks, uint64_t *first) {
    if (!ctx || (count && (!src || !dst))) return FBS_E_INVALID;
    if (!ctx->have_keys) return set_error(ctx, FBS_E_STATE, "fbs_keygen has not run");
    if ((checks & IO_SECRET) && ctx->eval_only) return set_error(ctx, FBS_E_STATE, EVAL_ONLY);
    int rc = FBS_OK;
    if ((checks & IO_BELOW_2_55) && (rc = check_nonces(ctx, *first, count))) return rc;
    if ((checks & IO_BELOW_2_56) && (rc = check_seeded_streams(ctx, *first, count))) return rc;
    if ((checks & IO_CT_WORDS) && (rc = check_ct_words(ctx, count))) return rc;
    if (checks & IO_FRESH) rc = reserve_fresh(ctx, count, first);
    return rc;
}

// compact and packed outputs: the width, and word counts that must not overflow
inline int check_bits(const fbs_ctx *ctx, uint32_t bits) {
    if (bits < ctx->p.log_n_poly + 1 || bits > 31) return set_error(ctx, FBS_E_INVALID, "compact width must lie in [log2(2N), 31]");
    return FBS_OK;
}
inline int check_compact_words(const fbs_ctx *ctx, size_t count, uint32_t bits) {
    if (count > SIZE_MAX / 8 / compact_words(ctx->p.n, bits)) return set_error(ctx, FBS_E_INVALID, "count * W words overflow");
    return FBS_OK;
}
// The gadget keys (GadgetKind, fbs_internal.hpp): what their entries check and answer, once for the packing key (both libraries)
// and the fold key (the GPU library).  The parameter range and the shapes are one (the accumulate kernel is the same one).
inline int check_gadget_params(const fbs_ctx *ctx, GadgetKind kind, uint32_t t, uint32_t gamma) {
    if (const char *why = gadget_params_refused(t, gamma)) return set_error(ctx, FBS_E_INVALID, gadget_text(kind, std::string("@ key needs ") + why));
    if (!pack_shape_built(ctx->p.log_n_poly, ctx->p.k)) return set_error(ctx, FBS_E_INVALID, gadget_text(kind, "no @ kernel for this (k, N)"));
    return FBS_OK;
}
// what a keygen checks before it draws anything, an import (`entry`: who makes the seeded keys it goes with) before it reads its
// bodies: the states in this order, then the parameters
inline int check_gadget_keygen(const fbs_ctx *ctx, GadgetKind kind, uint32_t t, uint32_t gamma, bool needs_secret = true,
                               const char *entry = "fbs_keygen_seeded") {
    if (!ctx) return FBS_E_INVALID;
    if (!ctx->have_keys) return set_error(ctx, FBS_E_STATE, "fbs_keygen has not run");
    if (needs_secret && ctx->eval_only) return set_error(ctx, FBS_E_STATE, EVAL_ONLY);
    if (!ctx->seeded_keys) return set_error(ctx, FBS_E_STATE, gadget_text(kind, "a @ key goes with seeded keys (") + entry + ")");
    return check_gadget_params(ctx, kind, t, gamma);
}
// the state change of a keygen or an import, once the key is where it is used (in the GPU library: on the device)
inline void gadget_key_in_place(fbs_ctx *ctx, GadgetKind kind, uint32_t t, uint32_t gamma, std::vector<uint64_t> &bodies) {
    HostState::GadgetKeyState &key = ctx->gadget[kind];
    key.bodies.swap(bodies);
    key.t = t;
    key.gamma = gamma;
    key.have = true;
}
// fbs_<noun>_key_sizes: words of the bodies and of the whole key at t levels (0: the context's own key)
inline int gadget_key_sizes(const fbs_ctx *ctx, GadgetKind kind, uint32_t t, size_t sizes[2]) {
    if (!ctx || !sizes) return FBS_E_INVALID;
    if (t == 0) {
        if (!ctx->gadget[kind].have) return set_error(ctx, FBS_E_STATE, gadget_text(kind, "the context has no @ key"));
        t = ctx->gadget[kind].t;
    }
    if (t > 31) return set_error(ctx, FBS_E_INVALID, gadget_text(kind, "@ key needs 1 <= t_# <= 31"));
    sizes[0] = (size_t)gadget_rows(*ctx, kind) * t * ctx->N;
    sizes[1] = sizes[0] * (ctx->p.k + 1);
    return FBS_OK;
}
// fbs_export_<noun>_key: the bodies, and (a test hook) the whole key in the coefficient domain
inline int gadget_key_export(const fbs_ctx *ctx, GadgetKind kind, uint64_t *bodies, uint64_t *full) {
    if (!ctx) return FBS_E_INVALID;
    const HostState::GadgetKeyState &key = ctx->gadget[kind];
    if (!key.have) return set_error(ctx, FBS_E_STATE, gadget_text(kind, "the context has no @ key"));
    if (bodies) std::memcpy(bodies, key.bodies.data(), key.bodies.size() * 8);
    if (full) {
        std::vector<uint64_t> whole;
        host_expand_gadget_key(ctx, kind, ctx->mask_key, key.t, key.bodies.data(), whole);
        std::memcpy(full, whole.data(), whole.size() * 8);
    }
    return FBS_OK;
}
inline int check_packed_words(const fbs_ctx *ctx, size_t count, uint32_t bits) {
    if (count / ctx->N + 1 > SIZE_MAX / 8 / packed_sample_words(ctx->p.k, ctx->N, ctx->N, bits))
        return set_error(ctx, FBS_E_INVALID, "packed words overflow");
    return FBS_OK;
}

}  // namespace fbs

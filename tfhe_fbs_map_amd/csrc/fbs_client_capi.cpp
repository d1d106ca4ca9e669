// extern "C" surface of libfbsclient.so, the part that differs on a machine with no GPU and no ROCm ("client library" in the
// header): a context is its host state (fbs::HostState) and nothing else, there is no device to name or to upload keys to.  The
// other entries the holder of the secret needs -- exports, encryption, decryption, the decoders of compact and packed outputs --
// are fbs_client_entries.cpp, the same text the GPU library is built from.  Every entry here does what its namesake in
// fbs_capi.cpp does up to the point where that one turns to the device: the same checks in the same order and the same state
// changes (fbs_api_checks.hpp), the same host functions (fbs_host.cpp).  Built with FBS_HOST_ONLY.
#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "fbs_api_checks.hpp"
#include "fbs_internal.hpp"

#ifndef FBS_HOST_ONLY
#error "fbs_client_capi.cpp belongs to the client library: build it with -DFBS_HOST_ONLY (make client)"
#endif

using namespace fbs;

// Parameter admission is the GPU library's.  Then the device: this library has none, and says so instead of ignoring an ordinal.
int fbs::ctx_create(const fbs_params *params, uint64_t seed, const uint8_t *seed32, int device, fbs_ctx **out) {
    if (!params || !out) return set_error(nullptr, FBS_E_INVALID, "null argument");
    *out = nullptr;
    fbs_ctx *admitted = nullptr;
    if (int rc = admit_params(params, seed, seed32, &admitted)) return rc;
    std::unique_ptr<fbs_ctx> ctx(admitted);
    if (device != FBS_DEVICE_NONE)
        return set_error(nullptr, FBS_E_DEVICE, "libfbsclient runs on the host only: pass device = FBS_DEVICE_NONE (-1); contexts on a "
                                                "GPU are libfbsexec.so's");
    *out = ctx.release();
    return FBS_OK;
}

extern "C" {

int fbs_ctx_create(const fbs_params *params, uint64_t seed, int device, fbs_ctx **out) try {
    return ctx_create(params, seed, nullptr, device, out);
} FBS_API_CATCH(nullptr)

int fbs_ctx_stat(const fbs_ctx *ctx, const char *name, int64_t *value) try {
    if (!ctx || !name || !value) return FBS_E_INVALID;
    const std::string k(name);
    if (!host_stat(ctx, k, value)) return set_error(ctx, FBS_E_INVALID, "unknown statistic '" + k + "'");
    return FBS_OK;
} FBS_API_CATCH(ctx)

void fbs_ctx_destroy(fbs_ctx *ctx) try {
    if (!ctx) return;
    // the secrets do not outlive the context in freed memory
    std::fill(ctx->sk_lwe.begin(), ctx->sk_lwe.end(), 0);
    std::fill(ctx->sk_glwe.begin(), ctx->sk_glwe.end(), 0);
    delete ctx;
} catch (...) {
}

const char *fbs_device_info(const fbs_ctx *) { return "host"; }

int fbs_keygen(fbs_ctx *ctx) try {
    if (!ctx) return FBS_E_INVALID;
    host_keygen(ctx);
    ctx->mask_key = mask_key_of(ctx->rkey);
    keys_replaced(ctx, false, false);
    keys_in_place(ctx);
    return FBS_OK;
} FBS_API_CATCH(ctx)

int fbs_keygen_seeded(fbs_ctx *ctx) try {
    if (!ctx) return FBS_E_INVALID;
    host_keygen_seeded(ctx);
    keys_replaced(ctx, true, false);
    keys_in_place(ctx);
    return FBS_OK;
} FBS_API_CATCH(ctx)

int fbs_packing_keygen(fbs_ctx *ctx, uint32_t t_p, uint32_t gamma_p) try {
    if (int rc = check_gadget_keygen(ctx, GK_PACK, t_p, gamma_p)) return rc;
    std::vector<uint64_t> bodies;
    host_gadget_keygen(ctx, GK_PACK, t_p, gamma_p, bodies);
    gadget_key_in_place(ctx, GK_PACK, t_p, gamma_p, bodies);
    return FBS_OK;
} FBS_API_CATCH(ctx)

}  // extern "C"

// extern "C" surface of libfbsexec.so (declared in include/fbs_exec.h): contexts, keys, inputs and outputs, the loaded program and
// its level calls.  The whole-program evaluations that stand behind `LutExecEnv.eval` are fbs_eval.cpp's.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>

#include "fbs_api_checks.hpp"
#include "fbs_compact.hpp"
#include "fbs_internal.hpp"
#include "fbs_pack.hpp"
#include "fbs_plan.hpp"

using namespace fbs;

// ---------------------------------------------------------------------------------------------
// program representation
// ---------------------------------------------------------------------------------------------
template <typename T>
static int to_device(fbs_ctx *ctx, fbs_prog *prog, const std::vector<T> &v, T **out) {
    *out = nullptr;
    if (v.empty()) return FBS_OK;
    void *d = nullptr;
    FBS_HIP(ctx, hipMalloc(&d, v.size() * sizeof(T)));
    prog->allocations.push_back(d);
    FBS_HIP(ctx, hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    *out = (T *)d;
    return FBS_OK;
}

// a LinearProd coefficient as the kernel wants it: centred residue, as the bit pattern of a double
static uint64_t coef_bits(int64_t c) {
    const double d = fq_centered(fq_from_i64(c));
    uint64_t u;
    std::memcpy(&u, &d, sizeof u);
    return u;
}

// ---- helpers of the entries, shared with fbs_eval.cpp (declared in fbs_internal.hpp) ------------------------------------------
namespace fbs {

hipStream_t pick(const fbs_ctx *ctx, void *stream) { return stream ? (hipStream_t)stream : ctx->stream; }

// Scratch is grown on demand, and growing it BLOCKS (the old buffers may still be read by queued kernels): a host that wants
// its *_dev calls to be nothing but kernel launches sizes everything up front with fbs_ctx_reserve.
int ensure_ms(fbs_ctx *ctx, size_t count) {
    if (int rc = dev_keyswitch_reserve(ctx, count)) return rc;   // (the int8-GEMM key switch's digit and limb-sum scratch)
    if (count <= ctx->ms_capacity) return FBS_OK;
    ctx->scratch_growths++;
    if (ctx->scratch_used) FBS_HIP(ctx, hipStreamSynchronize(ctx->scratch_stream));   // kernels may still read the old buffer
    for (void *p : {(void *)ctx->d_ms, (void *)ctx->d_ms_eps, (void *)ctx->d_ms_body})
        if (p) (void)hipFree(p);
    ctx->d_ms = nullptr;
    ctx->d_ms_eps = nullptr;
    ctx->d_ms_body = nullptr;
    ctx->ms_capacity = 0;
    FBS_HIP(ctx, hipMalloc(&ctx->d_ms, count * (ctx->p.n + 1) * sizeof(uint32_t)));
    FBS_HIP(ctx, hipMalloc(&ctx->d_ms_eps, count * 8));
    FBS_HIP(ctx, hipMalloc(&ctx->d_ms_body, count * 8));
    FBS_HIP(ctx, hipMemset(ctx->d_ms_eps, 0, count * 8));   // every launch leaves it zero again (k_ms_body)
    FBS_HIP(ctx, hipDeviceSynchronize());
    ctx->ms_capacity = count;
    return FBS_OK;
}

int ensure_acc(fbs_ctx *ctx, size_t rows) {   // a row = a whole GLWE accumulator
    return grow(ctx, ctx->d_acc, ctx->acc_capacity, rows, (size_t)(ctx->p.k + 1) * ctx->N * 8, true);
}
int ensure_wires(fbs_ctx *ctx, size_t words) { return grow(ctx, ctx->d_wires, ctx->wires_capacity, words, 8, true); }
static int ensure_audit(fbs_ctx *ctx, size_t rows, size_t words) {   // (not counted: an audit is not a hot path and always blocks)
    if (int rc = grow(ctx, ctx->d_audit_err, ctx->audit_err_capacity, words, 8, false)) return rc;
    return grow(ctx, ctx->d_audit_stats, ctx->audit_stats_capacity, rows, sizeof(fbs_audit_row), false);
}
int ensure_io_msgs(fbs_ctx *ctx, size_t words) { return grow(ctx, ctx->d_io_msgs, ctx->io_msgs_capacity, words, 8, true); }

// Cross-stream ordering of the per-context scratch (d_ms, d_idx, d_wires): a call on stream `s` first waits for the last
// call that used the scratch on ANOTHER stream; calls on one stream are ordered by the stream itself.
int scratch_wait(fbs_ctx *ctx, hipStream_t s) {
    if (ctx->scratch_used && ctx->scratch_stream != s) FBS_HIP(ctx, hipStreamWaitEvent(s, ctx->scratch_event, 0));
    return FBS_OK;
}
int scratch_done(fbs_ctx *ctx, hipStream_t s) {
    FBS_HIP(ctx, hipEventRecord(ctx->scratch_event, s));
    ctx->scratch_stream = s;
    ctx->scratch_used = true;
    return FBS_OK;
}

// A call that fails between scratch_wait and scratch_done may have left the "zero between launches" scratch (rounding-error
// sums, limb sums of the GEMM key switch) half used: put it back, so that the next call on the context starts clean.
int scratch_fail(fbs_ctx *ctx, hipStream_t s, int rc) {
    if (ctx->d_ms_eps && ctx->ms_capacity) (void)hipMemsetAsync(ctx->d_ms_eps, 0, ctx->ms_capacity * 8, s);
    (void)dev_keyswitch_rezero(ctx, s);
    (void)scratch_done(ctx, s);
    return rc;
}
// The bracket of every use of the scratch: wait, what `body` queues on `s`, then done -- or fail, with the code `body` gave
template <typename Body>
static int scratch_section(fbs_ctx *ctx, hipStream_t s, Body &&body) {
    if (int rc = scratch_wait(ctx, s)) return rc;
    if (int rc = body()) return scratch_fail(ctx, s, rc);
    return scratch_done(ctx, s);
}

// the plain batch: gate g = ciphertext g, one sample each
GateView batch_view(const uint64_t *in, uint64_t *out, const uint32_t *table_ids, size_t count) {
    GateView gv{};
    gv.in_base = in;
    gv.out_base = out;
    gv.table_ids = table_ids;
    gv.T = 1;
    gv.s_begin = 0;
    gv.s_count = 1;
    gv.f_begin = 0;
    gv.count = count;
    gv.ks_begin = 0;
    gv.ks_count = count;
    gv.n_gates = (uint32_t)count;
    return gv;
}

// `ng` wire slots (d_slot [ng], device) of a chunk of `tc` samples in a buffer of Tc a slot: gate g reads slot d_slot[g] of `in`
// and, `out` given, writes the same slot of `out`
GateView slots_view(const uint64_t *in, uint64_t *out, const uint32_t *d_slot, size_t ng, size_t Tc, size_t tc) {
    GateView gv{};   // (the window and both ranges start at 0)
    gv.in_base = in, gv.out_base = out, gv.src_slot = d_slot, gv.dst_slot = out ? d_slot : nullptr;
    gv.T = Tc, gv.s_count = tc, gv.count = gv.ks_count = ng * tc, gv.n_gates = (uint32_t)ng;
    return gv;
}

// `count` ciphertexts through the modulus-switch scratch in passes of what the context has of it, or of COMPACT_PASS when it has
// less: `pass(f0, rows)` queues ciphertexts [f0, f0 + rows) on `s`
size_t ms_pass_size(const fbs_ctx *ctx, size_t count) { return std::min(count, std::max(ctx->ms_capacity, COMPACT_PASS)); }
int ms_passes(fbs_ctx *ctx, size_t count, hipStream_t s, const std::function<int(size_t f0, size_t rows)> &pass) {
    const size_t per_pass = ms_pass_size(ctx, count);
    if (int rc = ensure_ms(ctx, per_pass)) return rc;
    return scratch_section(ctx, s, [&]() -> int {
        for (size_t f0 = 0; f0 < count; f0 += per_pass)
            if (int rc = pass(f0, std::min(per_pass, count - f0))) return rc;
        return FBS_OK;
    });
}

int sync_stream(fbs_ctx *ctx, hipStream_t s) {
    FBS_HIP(ctx, hipStreamSynchronize(s));
    return FBS_OK;
}

// what the entries that launch check first: the keys, the owner of a table set or a program, the device
static int check_ready(fbs_ctx *ctx, const fbs_tvset *tv) {
    if (!ctx) return FBS_E_INVALID;
    if (!ctx->have_keys) return set_error(ctx, FBS_E_STATE, "fbs_keygen has not run");
    if (tv && tv->ctx != ctx) return set_error(ctx, FBS_E_INVALID, "test-vector set belongs to another context");
    FBS_HIP(ctx, hipSetDevice(ctx->device));
    return FBS_OK;
}

int check_prog(fbs_ctx *ctx, const fbs_prog *prog) {
    int rc = check_ready(ctx, prog ? prog->tv : nullptr);
    if (rc != FBS_OK) return rc;
    if (!prog || prog->ctx != ctx) return set_error(ctx, FBS_E_INVALID, "program belongs to another context");
    return FBS_OK;
}

int ensure_idx(fbs_ctx *ctx, size_t words) {   // (not counted in scratch_growths)
    return words <= ctx->idx_capacity ? FBS_OK : grow(ctx, ctx->d_idx, ctx->idx_capacity, std::max<size_t>(words, 1 << 16), 4, false);
}

// the context's identity table [0, 1, .., p - 1], made on first use: a blind rotation through it is a refresh
int identity_tv(fbs_ctx *ctx, fbs_tvset **out) {
    if (!ctx->tv_identity) {
        std::vector<int32_t> vals(ctx->p.p_msg);
        for (uint32_t v = 0; v < ctx->p.p_msg; v++) vals[v] = (int32_t)v;
        const uint32_t off[2] = {0, ctx->p.p_msg};
        if (int rc = fbs_tvset_create(ctx, vals.data(), off, 1, &ctx->tv_identity)) return rc;
    }
    *out = ctx->tv_identity;
    return FBS_OK;
}

bool state_of(const fbs_ctx *ctx, const fbs_state *st) {   // (by address: a foreign or stale pointer is never dereferenced)
    return st && std::find(ctx->states.begin(), ctx->states.end(), st) != ctx->states.end();
}

// Parameter admission is host code with no device in it (admit_params: host_ctx_init of fbs_host.cpp, kernel_not_built of
// fbs_select.hpp; the sanitizer harnesses of tests/c/ run those two).  Then the device.
int ctx_create(const fbs_params *params, uint64_t seed, const uint8_t *seed32, int device, fbs_ctx **out) {
    if (!params || !out) return set_error(nullptr, FBS_E_INVALID, "null argument");
    *out = nullptr;
    fbs_ctx *admitted = nullptr;
    if (int rc = admit_params(params, seed, seed32, &admitted)) return rc;
    std::unique_ptr<fbs_ctx> ctx(admitted);
    ctx->device = device;

    int n_dev = 0;
    hipError_t e = hipGetDeviceCount(&n_dev);
    if (e != hipSuccess || n_dev <= 0)
        return set_error(nullptr, FBS_E_DEVICE, "no HIP device: libfbsexec has no CPU path (" + std::string(hipGetErrorString(e)) + ")");
    if (device < 0 || device >= n_dev) return set_error(nullptr, FBS_E_INVALID, "device ordinal out of range");
    e = hipSetDevice(device);
    if (e != hipSuccess) return set_error(nullptr, FBS_E_DEVICE, std::string("hipSetDevice: ") + hipGetErrorString(e));
    hipDeviceProp_t prop;
    e = hipGetDeviceProperties(&prop, device);
    if (e != hipSuccess) return set_error(nullptr, FBS_E_DEVICE, std::string("hipGetDeviceProperties: ") + hipGetErrorString(e));
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
        return set_error(nullptr, FBS_E_DEVICE, std::string("device is ") + prop.gcnArchName + "; this library carries gfx950 code only");
    ctx->cu_count = prop.multiProcessorCount;
    ctx->devinfo = std::string(prop.gcnArchName) + " " + prop.name + " CUs=" + std::to_string(prop.multiProcessorCount);
    // a blocking stream: ordered with the legacy null stream, which is what PyTorch's default stream is --
    // a caller that passes stream = NULL while using torch tensors still gets correct ordering
    e = hipStreamCreateWithFlags(&ctx->stream, hipStreamDefault);
    if (e != hipSuccess) return set_error(nullptr, FBS_E_DEVICE, std::string("hipStreamCreate: ") + hipGetErrorString(e));
    e = hipEventCreateWithFlags(&ctx->scratch_event, hipEventDisableTiming);
    if (e != hipSuccess) {
        (void)hipStreamDestroy(ctx->stream);
        return set_error(nullptr, FBS_E_DEVICE, std::string("hipEventCreate: ") + hipGetErrorString(e));
    }
    *out = ctx.release();
    return FBS_OK;
}

}   // namespace fbs

// The entries that never turn to the device (sizes, exports, host encryption and decryption, the decoders, fbs_last_error) are
// fbs_client_entries.cpp, one text for this library and the client library.
extern "C" {

// ---------------------------------------------------------------------------------------------
int fbs_ctx_create(const fbs_params *params, uint64_t seed, int device, fbs_ctx **out) try {
    return ctx_create(params, seed, nullptr, device, out);
} FBS_API_CATCH(nullptr)

int fbs_ctx_tune(fbs_ctx *ctx, const char *knob, int64_t value) try {
    if (!ctx || !knob) return FBS_E_INVALID;
    const std::string k(knob);
    int64_t *slot = tune_knob(ctx->tune, k);
    if (!slot) return set_error(ctx, FBS_E_INVALID, "unknown knob '" + k + "'");
    if (value < 0) return set_error(ctx, FBS_E_INVALID, "knob values are non-negative");
    *slot = value;
    return FBS_OK;
} FBS_API_CATCH(ctx)

int fbs_ctx_stat(const fbs_ctx *ctx, const char *name, int64_t *value) try {
    if (!ctx || !name || !value) return FBS_E_INVALID;
    const std::string k(name);
    if (host_stat(ctx, k, value)) return FBS_OK;   // (what the client library answers too)
    if (gadget_stat(ctx, GK_FOLD, k, value)) return FBS_OK;   // (folded state: this library's alone)
    if (k == "scratch_growths") *value = ctx->scratch_growths;
    else if (k == "ms_capacity") *value = (int64_t)ctx->ms_capacity;
    else if (k == "acc_capacity") *value = (int64_t)ctx->acc_capacity;
    else if (k == "wires_capacity") *value = (int64_t)ctx->wires_capacity;
    else if (k == "cu_count") *value = ctx->cu_count;
    else if (k == "states_alive") *value = (int64_t)ctx->states.size();
    else if (k == "state_bytes") *value = (int64_t)ctx->state_bytes;
    else if (k == "keys_made_on_device") *value = ctx->have_keys && ctx->keys_made_on_device;
    else if (k == "bsk_upload_bytes") *value = ctx->bsk_upload_bytes;
    else if (k == "lookup_tables") *value = ctx->lookup_tables;
    else if (k == "lookup_scratch_words") *value = (int64_t)ctx->lookup_tables_capacity;
    else if (k == "tables_alive") *value = (int64_t)ctx->tables.size();
    else if (k == "table_scratch_words") *value = (int64_t)ctx->table_scratch_capacity;
    else return set_error(ctx, FBS_E_INVALID, "unknown statistic '" + k + "'");
    return FBS_OK;
} FBS_API_CATCH(ctx)

int fbs_ctx_reserve(fbs_ctx *ctx, size_t max_keyswitches, size_t max_shared_rows, size_t wire_words) try {
    if (!ctx) return FBS_E_INVALID;
    FBS_HIP(ctx, hipSetDevice(ctx->device));
    int rc;
    if (max_keyswitches && (rc = ensure_ms(ctx, max_keyswitches)) != FBS_OK) return rc;
    if (max_shared_rows && (rc = ensure_acc(ctx, max_shared_rows)) != FBS_OK) return rc;
    if (wire_words && (rc = ensure_wires(ctx, wire_words)) != FBS_OK) return rc;
    return FBS_OK;
} FBS_API_CATCH(ctx)

void fbs_ctx_destroy(fbs_ctx *ctx) try {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx->scratch_used) (void)hipStreamSynchronize(ctx->scratch_stream);
    for (void *p : {(void *)ctx->d_bsk_hat, (void *)ctx->d_bsk_hat_small, (void *)ctx->d_ksk, (void *)ctx->d_ksk_f, (void *)ctx->d_ks_corr, (void *)ctx->d_ks_a, (void *)ctx->d_ks_b, (void *)ctx->d_ks_c, (void *)ctx->d_tw_fwd, (void *)ctx->d_tw_inv, (void *)ctx->d_psi_pow, (void *)ctx->d_ms, (void *)ctx->d_ms_eps, (void *)ctx->d_ms_body, (void *)ctx->d_acc, (void *)ctx->d_stage_in, (void *)ctx->d_stage_out, (void *)ctx->d_stage_ids,
                    (void *)ctx->d_idx, (void *)ctx->d_wires, (void *)ctx->d_sk_bits, (void *)ctx->d_sk_lwe_bits, (void *)ctx->d_io_msgs,
                    (void *)ctx->d_compact, (void *)ctx->d_links, (void *)ctx->d_pack_fields, (void *)ctx->d_pack_acc, (void *)ctx->d_pub, (void *)ctx->d_lookup_tables, (void *)ctx->d_lookup_idx, (void *)ctx->d_acc_flags, (void *)ctx->d_add_idx, (void *)ctx->d_table_scratch, (void *)ctx->d_audit_err, (void *)ctx->d_audit_stats})
        if (p) (void)hipFree(p);
    for (auto &key : ctx->gadget_dev)
        for (void *p : {(void *)key.d_key, (void *)key.d_out})
            if (p) (void)hipFree(p);
    for (fbs_state *st : ctx->states) {   // the states still alive
        (void)hipFree(st->d);
        delete st;
    }
    for (fbs_table *tab : ctx->tables) {   // ... and the tables
        (void)hipFree(tab->d);
        (void)hipFree(tab->d_unit_maps);
        delete tab;
    }
    if (ctx->inputs_event) (void)hipEventDestroy(ctx->inputs_event);
    fbs_tvset_destroy(ctx->tv_identity);
    if (ctx->scratch_event) (void)hipEventDestroy(ctx->scratch_event);
    for (auto &v : ctx->prof.pending)
        for (auto &pr : v) {
            (void)hipEventDestroy(pr.begin);
            (void)hipEventDestroy(pr.end);
        }
    for (auto &pr : ctx->prof.pool) {
        (void)hipEventDestroy(pr.first);
        (void)hipEventDestroy(pr.second);
    }
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
} catch (...) {   // (nothing here allocates; the promise of the ABI is kept anyway)
}

const char *fbs_device_info(const fbs_ctx *ctx) { return ctx ? ctx->devinfo.c_str() : ""; }

// ---------------------------------------------------------------------------------------------
// Keys on the device (knob "keys_on_device"): the secrets are drawn on the host and uploaded FIRST -- the kernels read them --, both
// evaluation keys are made there (bsk_bodies null) or expanded there from the bodies of a server key, the bootstrapping key is
// transformed straight from the device rows, and the rows come back as ctx->bsk / ctx->ksk: the exports and the key-switching
// tables (derived on the host, as ever) read those.
static int keys_on_device(fbs_ctx *ctx, bool seeded, const uint64_t *bsk_bodies, const uint64_t *ksk_bodies) {
    ctx->have_keys = false;
    int rc = bsk_bodies ? FBS_OK : dev_upload_secret(ctx);
    if (rc == FBS_OK) rc = dev_upload_tables(ctx);
    if (rc == FBS_OK) rc = dev_make_keys(ctx, seeded, ctx->mask_key, bsk_bodies, ksk_bodies);
    if (rc == FBS_OK) rc = dev_upload_ksk(ctx);
    if (rc != FBS_OK) return rc;
    ctx->bsk_upload_bytes = bsk_bodies ? (int64_t)(ctx->n_ggsw * ctx->rows * ctx->N * 8) : 0;
    return FBS_OK;
}

int fbs_keygen(fbs_ctx *ctx) try {
    if (!ctx) return FBS_E_INVALID;
    FBS_HIP(ctx, hipSetDevice(ctx->device));
    const bool on_device = ctx->tune.keys_on_device != 0;
    if (on_device) draw_secrets(ctx);
    else host_keygen(ctx);
    ctx->mask_key = mask_key_of(ctx->rkey);
    keys_replaced(ctx, false, false);
    int rc = on_device ? keys_on_device(ctx, false, nullptr, nullptr) : dev_upload_keys(ctx);
    if (rc == FBS_OK && !on_device) rc = dev_upload_secret(ctx);
    if (rc != FBS_OK) return rc;
    ctx->keys_made_on_device = on_device;
    keys_in_place(ctx);
    return FBS_OK;
} FBS_API_CATCH(ctx)

int fbs_import_keys(fbs_ctx *ctx, const uint64_t *sk_lwe, const uint64_t *sk_glwe, const uint64_t *bsk, const uint64_t *ksk) try {
    if (!ctx) return FBS_E_INVALID;
    if (!sk_lwe || !sk_glwe || !bsk || !ksk) return set_error(ctx, FBS_E_INVALID, "null argument");
    FBS_HIP(ctx, hipSetDevice(ctx->device));
    size_t sizes[4];
    fbs_key_sizes(ctx, sizes);
    for (size_t i = 0; i < sizes[0]; i++)
        if (sk_lwe[i] > 1) return set_error(ctx, FBS_E_INVALID, "secret keys are binary");
    for (size_t i = 0; i < sizes[1]; i++)
        if (sk_glwe[i] > 1) return set_error(ctx, FBS_E_INVALID, "secret keys are binary");
    for (size_t i = 0; i < sizes[2]; i++)
        if (bsk[i] >= FQ) return set_error(ctx, FBS_E_INVALID, "bootstrapping-key word is not a canonical residue");
    for (size_t i = 0; i < sizes[3]; i++)
        if (ksk[i] >= FQ) return set_error(ctx, FBS_E_INVALID, "key-switching-key word is not a canonical residue");
    if (const char *why = imported_keys_mismatch(ctx, sk_lwe, sk_glwe, bsk, ksk)) return set_error(ctx, FBS_E_INVALID, why);
    if (ctx->scratch_used) FBS_HIP(ctx, hipStreamSynchronize(ctx->scratch_stream));   // kernels may still read the old keys
    ctx->sk_lwe.assign(sk_lwe, sk_lwe + sizes[0]);
    ctx->sk_glwe.assign(sk_glwe, sk_glwe + sizes[1]);
    ctx->bsk.assign(bsk, bsk + sizes[2]);
    ctx->ksk.assign(ksk, ksk + sizes[3]);
    ctx->have_keys = false;
    ctx->mask_key = mask_key_of(ctx->rkey);
    keys_replaced(ctx, false, false);
    int rc = dev_upload_keys(ctx);
    if (rc == FBS_OK) rc = dev_upload_secret(ctx);
    if (rc != FBS_OK) return rc;
    ctx->keys_made_on_device = false;   // (the caller's keys: nothing to make)
    keys_in_place(ctx);
    return FBS_OK;
} FBS_API_CATCH(ctx)

// ---- the same on device buffers --------------------------------------------------------------
static IoView plain_rows(const int64_t *msgs, const uint64_t *cts, size_t count) {
    IoView v{};
    v.msgs = const_cast<int64_t *>(msgs);
    v.msg_stride = count;
    v.cts = const_cast<uint64_t *>(cts);
    v.ct_stride = count;
    v.rows = 1;
    v.per_row = count;
    return v;
}

int fbs_encrypt_dev(const fbs_ctx *ctx, const int64_t *d_msgs, size_t count, uint64_t nonce0, uint64_t *d_cts, void *stream) try {
    if (int rc = io_prologue(ctx, d_msgs, d_cts, count, IO_SECRET | IO_BELOW_2_55 | IO_CT_WORDS, &nonce0)) return rc;
    if (count == 0) return FBS_OK;
    FBS_HIP(ctx, hipSetDevice(ctx->device));
    return dev_encrypt(ctx, plain_rows(d_msgs, d_cts, count), nonce0, 0, pick(ctx, stream));
} FBS_API_CATCH(ctx)

int fbs_encrypt_fresh_dev(fbs_ctx *ctx, const int64_t *d_msgs, size_t count, uint64_t *d_cts, uint64_t *nonce0, void *stream) try {
    uint64_t first = 0;
    if (int rc = io_prologue(ctx, d_msgs, d_cts, count, IO_SECRET | IO_CT_WORDS | IO_FRESH, &first)) return rc;
    if (nonce0) *nonce0 = first;
    if (count == 0) return FBS_OK;
    FBS_HIP(ctx, hipSetDevice(ctx->device));
    return dev_encrypt(ctx, plain_rows(d_msgs, d_cts, count), first, 0, pick(ctx, stream));
} FBS_API_CATCH(ctx)

int fbs_decrypt_dev(const fbs_ctx *ctx, const uint64_t *d_cts, size_t count, int64_t *d_msgs, void *stream) try {
    if (int rc = io_prologue(ctx, d_cts, d_msgs, count, IO_SECRET | IO_CT_WORDS, nullptr)) return rc;
    if (count == 0) return FBS_OK;
    FBS_HIP(ctx, hipSetDevice(ctx->device));
    return dev_decrypt(ctx, plain_rows(d_msgs, d_cts, count), pick(ctx, stream));
} FBS_API_CATCH(ctx)

// ---- seeded keys and inputs: masks under a public key, only bodies travel ----------------------
int fbs_keygen_seeded(fbs_ctx *ctx) try {
    if (!ctx) return FBS_E_INVALID;
    FBS_HIP(ctx, hipSetDevice(ctx->device));
    const bool on_device = ctx->tune.keys_on_device != 0;
    if (on_device) {
        draw_secrets(ctx);
        ctx->mask_key = mask_key_of(ctx->rkey);
    } else {
        host_keygen_seeded(ctx);
    }
    keys_replaced(ctx, true, false);
    int rc = on_device ? keys_on_device(ctx, true, nullptr, nullptr) : dev_upload_keys(ctx);
    if (rc == FBS_OK && !on_device) rc = dev_upload_secret(ctx);
    if (rc != FBS_OK) return rc;
    ctx->keys_made_on_device = on_device;
    keys_in_place(ctx);
    return FBS_OK;
} FBS_API_CATCH(ctx)

int fbs_import_seeded_keys(fbs_ctx *ctx, const uint8_t mask_key[32], const uint64_t *bsk_bodies, const uint64_t *ksk_bodies) try {
    if (!ctx) return FBS_E_INVALID;
    if (!mask_key || !bsk_bodies || !ksk_bodies) return set_error(ctx, FBS_E_INVALID, "null argument");
    FBS_HIP(ctx, hipSetDevice(ctx->device));
    size_t sizes[2];
    fbs_seeded_key_sizes(ctx, sizes);
    for (size_t i = 0; i < sizes[0]; i++)
        if (bsk_bodies[i] >= FQ) return set_error(ctx, FBS_E_INVALID, "bootstrapping-key body word is not a canonical residue");
    for (size_t i = 0; i < sizes[1]; i++)
        if (ksk_bodies[i] >= FQ) return set_error(ctx, FBS_E_INVALID, "key-switching-key body word is not a canonical residue");
    RandKey mk;
    for (int i = 0; i < 8; i++)
        mk.w[i] = (uint32_t)mask_key[4 * i] | ((uint32_t)mask_key[4 * i + 1] << 8) | ((uint32_t)mask_key[4 * i + 2] << 16) |
                  ((uint32_t)mask_key[4 * i + 3] << 24);
    const bool on_device = ctx->tune.keys_on_device != 0;   // then only the bodies are uploaded, and expanded there
    std::vector<uint64_t> bsk, ksk;
    if (!on_device) host_expand_seeded_keys(ctx, mk, bsk_bodies, ksk_bodies, bsk, ksk);   // (the previous keys stay until this has succeeded)
    if (ctx->scratch_used) FBS_HIP(ctx, hipStreamSynchronize(ctx->scratch_stream));   // kernels may still read the old keys
    if (ctx->stream) FBS_HIP(ctx, hipStreamSynchronize(ctx->stream));               // ... or the old secret
    if (!on_device) {
        ctx->bsk.swap(bsk);
        ctx->ksk.swap(ksk);
    }
    std::fill(ctx->sk_lwe.begin(), ctx->sk_lwe.end(), 0);
    std::fill(ctx->sk_glwe.begin(), ctx->sk_glwe.end(), 0);
    std::vector<uint64_t>().swap(ctx->sk_lwe);
    std::vector<uint64_t>().swap(ctx->sk_glwe);
    for (uint32_t **bits : {&ctx->d_sk_bits, &ctx->d_sk_lwe_bits})
        if (*bits) {
            (void)hipFree(*bits);
            *bits = nullptr;
        }
    ctx->mask_key = mk;
    ctx->have_keys = false;
    keys_replaced(ctx, true, true);
    if (int rc = on_device ? keys_on_device(ctx, true, bsk_bodies, ksk_bodies) : dev_upload_keys(ctx)) return rc;
    ctx->keys_made_on_device = on_device;
    keys_in_place(ctx);
    return FBS_OK;
} FBS_API_CATCH(ctx)

int fbs_encrypt_seeded_dev(const fbs_ctx *ctx, const int64_t *d_msgs, size_t count, uint64_t nonce0, uint64_t *d_bodies, void *stream) try {
    if (int rc = io_prologue(ctx, d_msgs, d_bodies, count, IO_SECRET | IO_BELOW_2_55, &nonce0)) return rc;
    if (count == 0) return FBS_OK;
    FBS_HIP(ctx, hipSetDevice(ctx->device));
    return dev_encrypt_seeded(ctx, d_msgs, count, nonce0, d_bodies, pick(ctx, stream));
} FBS_API_CATCH(ctx)

int fbs_encrypt_seeded_fresh_dev(fbs_ctx *ctx, const int64_t *d_msgs, size_t count, uint64_t *d_bodies, uint64_t *nonce0, void *stream) try {
    uint64_t first = 0;
    if (int rc = io_prologue(ctx, d_msgs, d_bodies, count, IO_SECRET | IO_FRESH, &first)) return rc;
    if (nonce0) *nonce0 = first;
    if (count == 0) return FBS_OK;
    FBS_HIP(ctx, hipSetDevice(ctx->device));
    return dev_encrypt_seeded(ctx, d_msgs, count, first, d_bodies, pick(ctx, stream));
} FBS_API_CATCH(ctx)

int fbs_expand_seeded_dev(const fbs_ctx *ctx, const uint64_t *d_bodies, size_t count, uint64_t nonce0, uint64_t *d_cts, void *stream) try {
    if (int rc = io_prologue(ctx, d_bodies, d_cts, count, IO_BELOW_2_56 | IO_CT_WORDS, &nonce0)) return rc;
    if (count == 0) return FBS_OK;
    FBS_HIP(ctx, hipSetDevice(ctx->device));
    IoView v = plain_rows(nullptr, d_cts, count);
    v.msgs = reinterpret_cast<int64_t *>(const_cast<uint64_t *>(d_bodies));
    return dev_expand_seeded(ctx, v, nonce0, 0, pick(ctx, stream));
} FBS_API_CATCH(ctx)

// ---------------------------------------------------------------------------------------------
int fbs_tvset_create(fbs_ctx *ctx, const int32_t *table_vals, const uint32_t *table_off, uint32_t n_tables, fbs_tvset **out) try {
    if (!ctx || !out || (n_tables && (!table_vals || !table_off))) return FBS_E_INVALID;
    *out = nullptr;
    // the count is checked BEFORE anything is sized by it: more than 2^20 tables (8 GB of test vectors at N = 1024) is a
    // corrupted count, not a program
    if (n_tables > FBS_MAX_TABLES) return set_error(ctx, FBS_E_INVALID, "more than FBS_MAX_TABLES tables");
    FBS_HIP(ctx, hipSetDevice(ctx->device));
    std::unique_ptr<fbs_tvset> tv(new fbs_tvset);
    tv->ctx = ctx;
    tv->n_tables = n_tables;
    const uint32_t N = ctx->N;
    // the tables, then TV_0 (index n_tables): what a rotation shared by several tables starts from
    std::vector<uint64_t> host((size_t)(n_tables + 1) * N, 0);
    tv->post.assign((size_t)n_tables + 1, 0);
    tv->diff_cap = ctx->p.p_msg + 1;
    std::vector<uint32_t> dpos((size_t)std::max(1u, n_tables) * tv->diff_cap, 0), dn(std::max(1u, n_tables), 0);
    std::vector<int32_t> dval((size_t)std::max(1u, n_tables) * tv->diff_cap, 0);
    tv->diff_norm2.assign(n_tables, 0);
    tv->g_norm2.assign(n_tables, 0);
    tv->fusable.assign(n_tables, 0);
    for (uint32_t t = 0; t < n_tables; t++) {
        if (table_off[t + 1] < table_off[t]) return set_error(ctx, FBS_E_INVALID, "table offsets must be non-decreasing");
        const int32_t *vals = table_vals + table_off[t];
        const uint32_t len = table_off[t + 1] - table_off[t];
        int rc = host_build_tv(ctx, vals, len, host.data() + (size_t)t * N, &tv->post[t]);
        uint64_t abs_sum = 0;
        if (rc == FBS_OK)
            rc = host_build_tv_diff(ctx, vals, len, dpos.data() + (size_t)t * tv->diff_cap, dval.data() + (size_t)t * tv->diff_cap, &dn[t],
                                    &tv->diff_norm2[t], &tv->g_norm2[t], &abs_sum);
        if (rc != FBS_OK)
            return set_error(ctx, rc, "table " + std::to_string(t) + " of length " + std::to_string(len) +
                                          " is not evaluable by one bootstrap at p = " + std::to_string(ctx->p.p_msg));
        tv->fusable[t] = abs_sum < (1ull << 16);   // k_multi_extract sums d * word (< 2^46) in 64 bits
    }
    for (uint32_t j = 0; j < N; j++) host[(size_t)n_tables * N + j] = ctx->delta_half;
    hipError_t e = hipMalloc(&tv->d_tvs, host.size() * 8);
    if (e == hipSuccess) e = hipMalloc(&tv->d_post, tv->post.size() * 8);
    if (e == hipSuccess) e = hipMalloc(&tv->d_diff_pos, dpos.size() * 4);
    if (e == hipSuccess) e = hipMalloc(&tv->d_diff_val, dval.size() * 4);
    if (e == hipSuccess) e = hipMalloc(&tv->d_diff_n, dn.size() * 4);
    if (e == hipSuccess) e = hipMemcpy(tv->d_tvs, host.data(), host.size() * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(tv->d_post, tv->post.data(), tv->post.size() * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(tv->d_diff_pos, dpos.data(), dpos.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(tv->d_diff_val, dval.data(), dval.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(tv->d_diff_n, dn.data(), dn.size() * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        fbs_tvset_destroy(tv.release());   // frees whichever buffer was obtained
        return set_error(ctx, FBS_E_DEVICE, std::string("test-vector upload: ") + hipGetErrorString(e));
    }
    *out = tv.release();
    return FBS_OK;
} FBS_API_CATCH(ctx)

int fbs_table_fusion_norms(const fbs_tvset *tv, uint32_t table, uint64_t *d_norm2, uint64_t *g_norm2) try {
    if (!tv || table >= tv->n_tables) return FBS_E_INVALID;
    if (d_norm2) *d_norm2 = tv->diff_norm2[table];
    if (g_norm2) *g_norm2 = tv->g_norm2[table];
    return FBS_OK;
} FBS_API_CATCH(tv ? tv->ctx : nullptr)

void fbs_tvset_destroy(fbs_tvset *tv) try {
    if (!tv) return;
    if (tv->ctx) (void)hipSetDevice(tv->ctx->device);
    if (tv->d_tvs) (void)hipFree(tv->d_tvs);
    if (tv->d_post) (void)hipFree(tv->d_post);
    if (tv->d_diff_pos) (void)hipFree(tv->d_diff_pos);
    if (tv->d_diff_val) (void)hipFree(tv->d_diff_val);
    if (tv->d_diff_n) (void)hipFree(tv->d_diff_n);
    delete tv;
} catch (...) {   // (nothing here allocates; the promise of the ABI is kept anyway)
}

// ---------------------------------------------------------------------------------------------
int fbs_bootstrap_batch_dev(fbs_ctx *ctx, const fbs_tvset *tv, const uint64_t *d_cts_in, const uint32_t *d_table_ids,
                            size_t count, uint64_t *d_cts_out, void *stream) try {
    int rc = check_ready(ctx, tv);
    if (rc != FBS_OK) return rc;
    if (!tv || (count && (!d_cts_in || !d_cts_out))) return set_error(ctx, FBS_E_INVALID, "null argument");
    if (count == 0) return FBS_OK;
    if (count > 0x7FFFFFFFull) return set_error(ctx, FBS_E_INVALID, "batch too large");
    rc = ensure_ms(ctx, count);
    if (rc != FBS_OK) return rc;
    const GateView gv = batch_view(d_cts_in, d_cts_out, d_table_ids, count);
    hipStream_t s = pick(ctx, stream);
    return scratch_section(ctx, s, [&]() -> int {
        if (int rc = dev_keyswitch(ctx, gv, ctx->d_ms, ctx->p.log_n_poly + 1, s)) return rc;
        return dev_blind_rotate(ctx, tv, gv, ctx->d_ms, s);
    });
} FBS_API_CATCH(ctx)

int fbs_bootstrap_batch(fbs_ctx *ctx, const fbs_tvset *tv, const uint64_t *cts_in, const uint32_t *table_ids, size_t count,
                        uint64_t *cts_out) try {
    int rc = check_ready(ctx, tv);
    if (rc != FBS_OK) return rc;
    if (!tv || (count && (!cts_in || !cts_out))) return set_error(ctx, FBS_E_INVALID, "null argument");
    if (count == 0) return FBS_OK;
    if (table_ids)
        for (size_t i = 0; i < count; i++)
            if (table_ids[i] >= tv->n_tables) return set_error(ctx, FBS_E_INVALID, "table id out of range");
    // device staging owned by the context (grown on demand, reused from call to call: no allocation on the steady path)
    const size_t words = count * (ctx->D + 1);
    if (ctx->stage_capacity < count) {
        if (ctx->scratch_used) FBS_HIP(ctx, hipStreamSynchronize(ctx->scratch_stream));
        for (void *p : {(void *)ctx->d_stage_in, (void *)ctx->d_stage_out, (void *)ctx->d_stage_ids})
            if (p) (void)hipFree(p);
        ctx->d_stage_in = ctx->d_stage_out = nullptr;
        ctx->d_stage_ids = nullptr;
        ctx->stage_capacity = 0;
        FBS_HIP(ctx, hipMalloc(&ctx->d_stage_in, words * 8));
        FBS_HIP(ctx, hipMalloc(&ctx->d_stage_out, words * 8));
        FBS_HIP(ctx, hipMalloc(&ctx->d_stage_ids, count * 4));
        ctx->stage_capacity = count;
    }
    hipStream_t s = ctx->stream;
    rc = scratch_section(ctx, s, [&]() -> int {   // the staging buffers are per-context scratch too
        FBS_HIP(ctx, hipMemcpyAsync(ctx->d_stage_in, cts_in, words * 8, hipMemcpyHostToDevice, s));
        if (table_ids) FBS_HIP(ctx, hipMemcpyAsync(ctx->d_stage_ids, table_ids, count * 4, hipMemcpyHostToDevice, s));
        return FBS_OK;
    });
    if (rc != FBS_OK) return rc;
    rc = fbs_bootstrap_batch_dev(ctx, tv, ctx->d_stage_in, table_ids ? ctx->d_stage_ids : nullptr, count, ctx->d_stage_out, nullptr);
    if (rc != FBS_OK) {
        (void)hipStreamSynchronize(s);
        return rc;
    }
    FBS_HIP(ctx, hipMemcpyAsync(cts_out, ctx->d_stage_out, words * 8, hipMemcpyDeviceToHost, s));
    FBS_HIP(ctx, hipStreamSynchronize(s));
    return FBS_OK;
} FBS_API_CATCH(ctx)

// ---------------------------------------------------------------------------------------------
// wire-slot building blocks with HOST index arrays (convenience: each call stages its indices through a
// per-context buffer and waits for the copy; hosts that step a loaded program use the fbs_level_* calls below,
// whose index arrays were uploaded once by fbs_program_load)
// ---------------------------------------------------------------------------------------------
int fbs_lincomb_dev(fbs_ctx *ctx, uint64_t *d_wires, size_t T, uint32_t n_out, const uint32_t *dst, const uint32_t *term_off,
                    const uint32_t *srcs, const int64_t *coefs, const int64_t *consts, void *stream) try {
    int rc = check_ready(ctx, nullptr);
    if (rc != FBS_OK) return rc;
    if (n_out == 0 || T == 0) return FBS_OK;
    if (!d_wires || !dst || !term_off || !consts) return set_error(ctx, FBS_E_INVALID, "null argument");
    const uint32_t n_terms = term_off[n_out];
    if (n_terms && (!srcs || !coefs)) return set_error(ctx, FBS_E_INVALID, "null argument");
    // staging: [dst n_out][term_off n_out+1][srcs n_terms] as u32, then coefs and consts as u64
    size_t u32_words = (size_t)n_out + (n_out + 1) + n_terms;
    u32_words = (u32_words + 1) & ~(size_t)1;
    size_t total = u32_words + 2 * ((size_t)n_terms + n_out);
    hipStream_t s = pick(ctx, stream);
    if (ctx->scratch_used) FBS_HIP(ctx, hipStreamSynchronize(ctx->scratch_stream));   // the staging buffer may still be read
    rc = ensure_idx(ctx, total);
    if (rc != FBS_OK) return rc;
    std::vector<uint32_t> stage(total, 0);
    std::memcpy(stage.data(), dst, (size_t)n_out * 4);
    std::memcpy(stage.data() + n_out, term_off, (size_t)(n_out + 1) * 4);
    if (n_terms) std::memcpy(stage.data() + 2 * (size_t)n_out + 1, srcs, (size_t)n_terms * 4);
    uint64_t *f = reinterpret_cast<uint64_t *>(stage.data() + u32_words);
    for (uint32_t i = 0; i < n_terms; i++) f[i] = coef_bits(coefs[i]);
    for (uint32_t g = 0; g < n_out; g++) f[n_terms + g] = fq_mul(fq_from_i64(consts[g]), 2 * ctx->delta_half);
    FBS_HIP(ctx, hipMemcpyAsync(ctx->d_idx, stage.data(), total * 4, hipMemcpyHostToDevice, s));
    FBS_HIP(ctx, hipStreamSynchronize(s));   // `stage` is pageable host memory going out of scope
    const uint32_t *d_dst = ctx->d_idx, *d_off = ctx->d_idx + n_out, *d_srcs = ctx->d_idx + 2 * (size_t)n_out + 1;
    const uint64_t *d_f = reinterpret_cast<const uint64_t *>(ctx->d_idx + u32_words);
    rc = dev_lincomb(ctx, d_wires, T, 0, T, n_out, d_dst, d_off, d_srcs, d_f, d_f + n_terms, s);
    if (rc != FBS_OK) return rc;
    return scratch_done(ctx, s);
} FBS_API_CATCH(ctx)

int fbs_bootstrap_wires_dev(fbs_ctx *ctx, const fbs_tvset *tv, uint64_t *d_wires, size_t T, uint32_t n_gates,
                            const uint32_t *src, const uint32_t *dst, const uint32_t *table_ids, size_t s_begin, size_t s_end,
                            void *stream) try {
    int rc = check_ready(ctx, tv);
    if (rc != FBS_OK) return rc;
    if (!tv || !d_wires || !src || !dst || !table_ids) return set_error(ctx, FBS_E_INVALID, "null argument");
    if (s_end > T || s_begin > s_end) return set_error(ctx, FBS_E_INVALID, "bad sample range");
    if (n_gates == 0 || s_begin == s_end) return FBS_OK;
    for (uint32_t g = 0; g < n_gates; g++)
        if (table_ids[g] >= tv->n_tables) return set_error(ctx, FBS_E_INVALID, "table id out of range");
    const size_t count = (size_t)n_gates * (s_end - s_begin);
    hipStream_t s = pick(ctx, stream);
    if (ctx->scratch_used) FBS_HIP(ctx, hipStreamSynchronize(ctx->scratch_stream));
    rc = ensure_idx(ctx, 3 * (size_t)n_gates);
    if (rc != FBS_OK) return rc;
    rc = ensure_ms(ctx, count);
    if (rc != FBS_OK) return rc;
    std::vector<uint32_t> stage(3 * (size_t)n_gates);
    std::memcpy(stage.data(), src, (size_t)n_gates * 4);
    std::memcpy(stage.data() + n_gates, dst, (size_t)n_gates * 4);
    std::memcpy(stage.data() + 2 * (size_t)n_gates, table_ids, (size_t)n_gates * 4);
    FBS_HIP(ctx, hipMemcpyAsync(ctx->d_idx, stage.data(), stage.size() * 4, hipMemcpyHostToDevice, s));
    FBS_HIP(ctx, hipStreamSynchronize(s));
    GateView gv{};
    gv.in_base = d_wires;
    gv.out_base = d_wires;
    gv.src_slot = ctx->d_idx;
    gv.dst_slot = ctx->d_idx + n_gates;
    gv.table_ids = ctx->d_idx + 2 * (size_t)n_gates;
    gv.T = T;
    gv.s_begin = s_begin;
    gv.s_count = s_end - s_begin;
    gv.f_begin = 0;
    gv.count = count;
    gv.ks_begin = 0;
    gv.ks_count = count;
    gv.n_gates = n_gates;
    rc = dev_keyswitch(ctx, gv, ctx->d_ms, ctx->p.log_n_poly + 1, s);
    if (rc != FBS_OK) return rc;
    rc = dev_blind_rotate(ctx, tv, gv, ctx->d_ms, s);
    if (rc != FBS_OK) return rc;
    return scratch_done(ctx, s);
} FBS_API_CATCH(ctx)

// ---------------------------------------------------------------------------------------------
// whole-program executor
// ---------------------------------------------------------------------------------------------
int fbs_program_load(fbs_ctx *ctx, const fbs_program_desc *d, const fbs_tvset *tv, fbs_prog **out) try {
    return fbs_program_load_ex(ctx, d, tv, 0, out);
} FBS_API_CATCH(ctx)

int fbs_program_load_ex(fbs_ctx *ctx, const fbs_program_desc *d, const fbs_tvset *tv, uint32_t flags, fbs_prog **out) try {
    int rc = check_ready(ctx, tv);
    if (rc != FBS_OK) return rc;
    if (!d || !out) return set_error(ctx, FBS_E_INVALID, "null argument");
    *out = nullptr;
    if (flags & ~(uint32_t)FBS_LOAD_FUSE_TABLES) return set_error(ctx, FBS_E_INVALID, "unknown load flag");
    // the schedule: levels, wire slots by liveness, stage tables -- host arithmetic with no device in it (fbs_plan.cpp; the same
    // function runs under the sanitizers in tests/c/host_harness.cpp)
    ProgramPlan plan;
    std::string why;
    const bool fuse = (flags & FBS_LOAD_FUSE_TABLES) != 0;
    if (plan_program(d, tv ? tv->n_tables : 0u, fuse && tv ? tv->fusable.data() : nullptr, &plan, &why) != FBS_OK)
        return set_error(ctx, FBS_E_INVALID, why);
    std::unique_ptr<fbs_prog, void (*)(fbs_prog *)> prog(new fbs_prog, fbs_program_destroy);
    prog->fused = fuse;
    prog->ctx = ctx;
    prog->tv = tv;
    prog->n_inputs = d->n_inputs;
    prog->n_instr = d->n_instr;
    prog->n_outputs = d->n_outputs;
    prog->n_wires = plan.n_wires;
    prog->n_slots = plan.n_slots;
    prog->depth = plan.depth;
    prog->max_width = plan.max_width;
    prog->max_sources = plan.max_sources;
    prog->max_shared = plan.max_shared;
    prog->n_bootstrap = plan.n_bootstrap;
    prog->n_keyswitch = plan.n_keyswitch;
    prog->n_rotations = plan.n_rotations;
    prog->in_slot = plan.in_slot;
    prog->out_slot = plan.out_slot;
    {
        std::vector<uint32_t> out_slot(plan.out_slot.size());
        for (size_t o = 0; o < out_slot.size(); o++) out_slot[o] = plan.out_slot[o] >= 0 ? (uint32_t)plan.out_slot[o] : 0xFFFFFFFFu;
        if ((rc = to_device(ctx, prog.get(), plan.in_slot, &prog->d_in_slot)) || (rc = to_device(ctx, prog.get(), out_slot, &prog->d_out_slot)))
            return rc;
        std::vector<uint32_t> live_slot;
        for (size_t o = 0; o < out_slot.size(); o++)
            if (plan.out_slot[o] >= 0) {
                prog->live_out.push_back((uint32_t)o);
                live_slot.push_back(out_slot[o]);
            }
        if ((rc = to_device(ctx, prog.get(), live_slot, &prog->d_live_slot))) return rc;
    }
    // ---- upload the stage tables (coefficients and constants mapped into the field) ----------------------------------
    prog->lin.resize(plan.depth + 1);
    prog->boot.resize(plan.depth);
    for (uint32_t L = 0; L <= plan.depth; L++) {
        for (const LinPlan &h : plan.lin[L]) {
            LincombStage st;
            st.n_out = (uint32_t)h.dst.size();
            std::vector<uint64_t> coefs(h.coefs.size()), consts(h.consts.size());
            for (size_t i = 0; i < coefs.size(); i++) coefs[i] = coef_bits(h.coefs[i]);
            for (size_t i = 0; i < consts.size(); i++) consts[i] = fq_mul(fq_from_i64(h.consts[i]), 2 * ctx->delta_half);
            if (st.n_out &&
                ((rc = to_device(ctx, prog.get(), h.dst, &st.d_dst)) || (rc = to_device(ctx, prog.get(), h.off, &st.d_term_off)) ||
                 (rc = to_device(ctx, prog.get(), h.srcs, &st.d_srcs)) || (rc = to_device(ctx, prog.get(), coefs, &st.d_coefs)) ||
                 (rc = to_device(ctx, prog.get(), consts, &st.d_consts))))
                return rc;
            prog->lin[L].push_back(st);   // kept even when empty: the plan's stage times count every sub-stage
        }
    }
    for (uint32_t L = 0; L < plan.depth; L++) {
        const BootPlan &h = plan.boot[L];
        BootStage st;
        st.n_gates = (uint32_t)h.dst.size();
        st.n_sources = (uint32_t)h.src_slot.size();
        st.n_shared = h.n_shared;
        st.n_extract = (uint32_t)h.x_row.size();
        st.source_of = h.source_of;
        if ((rc = to_device(ctx, prog.get(), h.src_slot, &st.d_src_slot)) || (rc = to_device(ctx, prog.get(), h.source_of, &st.d_source_of)) ||
            (rc = to_device(ctx, prog.get(), h.dst, &st.d_dst)) || (rc = to_device(ctx, prog.get(), h.table, &st.d_table)))
            return rc;
        if (st.n_extract && ((rc = to_device(ctx, prog.get(), h.x_row, &st.d_x_row)) || (rc = to_device(ctx, prog.get(), h.x_table, &st.d_x_table)) ||
                             (rc = to_device(ctx, prog.get(), h.x_dst, &st.d_x_dst)) || (rc = to_device(ctx, prog.get(), h.x_gate, &st.d_x_gate))))
            return rc;
        prog->boot[L] = std::move(st);
    }
    // ---- what the audit reports (fbs_audit_rows): wire id and slot of every row of every (level, point) ---------------------
    prog->audit_lin.resize(plan.depth + 1);
    prog->audit_boot.resize(plan.depth);
    prog->audit_src.resize(plan.depth);
    for (uint32_t L = 0; L <= plan.depth; L++) {
        // a LinearProd that only an earlier sub-stage of its level reads may have lent its slot to a later one: the rows are the
        // wires their slot still holds once every sub-stage has run
        std::vector<uint32_t> holder(plan.n_slots, 0xFFFFFFFFu), slots;
        for (const LinPlan &h : plan.lin[L])
            for (size_t o = 0; o < h.dst.size(); o++) holder[h.dst[o]] = h.dst_wire[o];
        for (const LinPlan &h : plan.lin[L])
            for (size_t o = 0; o < h.dst.size(); o++)
                if (holder[h.dst[o]] == h.dst_wire[o]) {
                    prog->audit_lin[L].wire.push_back(h.dst_wire[o]);
                    slots.push_back(h.dst[o]);
                }
        if ((rc = to_device(ctx, prog.get(), slots, &prog->audit_lin[L].d_slot))) return rc;
    }
    for (uint32_t L = 0; L < plan.depth; L++) {
        const BootPlan &h = plan.boot[L];
        std::vector<uint32_t> slots;
        for (size_t g = 0; g < h.dst.size(); g++)
            if (h.dst_wire[g] != 0xFFFFFFFFu) {   // (a shared rotation writes no wire)
                prog->audit_boot[L].wire.push_back(h.dst_wire[g]);
                slots.push_back(h.dst[g]);
            }
        for (size_t e = 0; e < h.x_dst.size(); e++) {
            prog->audit_boot[L].wire.push_back(h.x_wire[e]);
            slots.push_back(h.x_dst[e]);
        }
        if ((rc = to_device(ctx, prog.get(), slots, &prog->audit_boot[L].d_slot))) return rc;
        prog->audit_src[L] = h.src_wire;
    }
    *out = prog.release();
    return FBS_OK;
} FBS_API_CATCH(ctx)

void fbs_program_destroy(fbs_prog *prog) try {
    if (!prog) return;
    if (prog->ctx) (void)hipSetDevice(prog->ctx->device);
    for (void *p : prog->allocations) (void)hipFree(p);
    delete prog;
} catch (...) {   // (nothing here allocates; the promise of the ABI is kept anyway)
}

int fbs_program_info(const fbs_prog *prog, uint32_t *n_levels, uint32_t *max_width, uint32_t *n_bootstrap) try {
    if (!prog) return FBS_E_INVALID;
    if (n_levels) *n_levels = prog->depth;
    if (max_width) *max_width = prog->max_width;
    if (n_bootstrap) *n_bootstrap = prog->n_bootstrap;
    return FBS_OK;
} FBS_API_CATCH(prog ? prog->ctx : nullptr)

int fbs_program_layout(const fbs_prog *prog, fbs_layout *out) try {
    if (!prog || !out) return FBS_E_INVALID;
    out->n_slots = prog->n_slots;
    out->n_levels = prog->depth;
    out->max_width = prog->max_width;
    out->max_sources = prog->max_sources;
    out->n_bootstrap = prog->n_bootstrap;
    out->n_keyswitch = prog->n_keyswitch;
    out->n_rotations = prog->n_rotations;
    out->row_words = prog->fused ? (prog->ctx->p.k + 1) * prog->ctx->N : prog->ctx->D + 1;
    out->n_inputs = prog->n_inputs;
    out->n_outputs = prog->n_outputs;
    return FBS_OK;
} FBS_API_CATCH(prog ? prog->ctx : nullptr)

int fbs_program_level(const fbs_prog *prog, uint32_t level, uint32_t *n_gates, uint32_t *n_sources) try {
    if (!prog || level >= prog->depth) return FBS_E_INVALID;
    if (n_gates) *n_gates = prog->boot[level].n_gates;
    if (n_sources) *n_sources = prog->boot[level].n_sources;
    return FBS_OK;
} FBS_API_CATCH(prog ? prog->ctx : nullptr)

int fbs_program_io_slots(const fbs_prog *prog, uint32_t *in_slot, int64_t *out_slot) try {
    if (!prog) return FBS_E_INVALID;
    if (in_slot) std::copy(prog->in_slot.begin(), prog->in_slot.end(), in_slot);
    if (out_slot) std::copy(prog->out_slot.begin(), prog->out_slot.end(), out_slot);
    return FBS_OK;
} FBS_API_CATCH(prog ? prog->ctx : nullptr)

// ---- one level at a time, device-resident wires, nothing but kernel launches on `stream` ------------------------
static int check_level_call(fbs_ctx *ctx, const fbs_prog *prog, const uint64_t *d_wires, size_t T, size_t s_begin, size_t s_count) {
    if (int rc = check_prog(ctx, prog)) return rc;
    if (!d_wires) return set_error(ctx, FBS_E_INVALID, "null argument");
    if (s_begin + s_count > T) return set_error(ctx, FBS_E_INVALID, "bad sample range");
    return FBS_OK;
}

int fbs_level_lincomb_dev(fbs_ctx *ctx, const fbs_prog *prog, uint32_t level, uint64_t *d_wires, size_t T, size_t s_begin,
                          size_t s_count, void *stream) try {
    int rc = check_level_call(ctx, prog, d_wires, T, s_begin, s_count);
    if (rc != FBS_OK) return rc;
    if (level > prog->depth) return set_error(ctx, FBS_E_INVALID, "level out of range");
    hipStream_t s = pick(ctx, stream);
    for (const LincombStage &st : prog->lin[level]) {
        rc = dev_lincomb(ctx, d_wires, T, s_begin, s_count, st.n_out, st.d_dst, st.d_term_off, st.d_srcs, st.d_coefs, st.d_consts, s);
        if (rc != FBS_OK) return rc;
    }
    return FBS_OK;
} FBS_API_CATCH(ctx)

// bootstraps [f_begin, f_end) (f_begin < f_end) of level stage `b` over samples [s_begin, s_begin + s_count), as the launchers see them
static GateView level_view(const fbs_ctx *ctx, const fbs_prog *prog, const BootStage &b, uint64_t *d_wires, uint64_t *d_rows, size_t T,
                           size_t s_begin, size_t s_count, size_t f_begin, size_t f_end) {
    // the key switches this slice needs: the (source, sample) pairs of its gates, as ONE flattened range.  Gates are
    // sorted by source, so only the first and the last gate of the slice can be cut short in the sample direction, and
    // only while no other gate of the slice shares their source.
    const size_t g0 = f_begin / s_count, s0 = f_begin % s_count;
    const size_t g1 = (f_end - 1) / s_count, s1 = (f_end - 1) % s_count + 1;
    const size_t u0 = b.source_of[g0], u1 = b.source_of[g1];
    const bool first_shared = g1 > g0 && b.source_of[g0 + 1] == u0;
    const bool last_shared = g1 > g0 && b.source_of[g1 - 1] == u1;
    GateView gv{};
    gv.in_base = d_wires;
    gv.out_base = d_wires;
    gv.src_slot = b.d_src_slot;
    gv.dst_slot = b.d_dst;
    gv.table_ids = b.d_table;
    gv.source_of = b.d_source_of;
    gv.out_rows = d_rows;
    gv.row_words = (d_rows && prog->fused) ? (ctx->p.k + 1) * ctx->N : 0;
    gv.T = T;
    gv.s_begin = s_begin;
    gv.s_count = s_count;
    gv.f_begin = f_begin;
    gv.count = f_end - f_begin;
    gv.ks_begin = u0 * s_count + (first_shared ? 0 : s0);
    gv.ks_count = u1 * s_count + (last_shared ? s_count : s1) - gv.ks_begin;
    gv.n_gates = b.n_gates;
    return gv;
}

int fbs_level_bootstrap_dev(fbs_ctx *ctx, const fbs_prog *prog, uint32_t level, uint64_t *d_wires, size_t T, size_t s_begin,
                            size_t s_count, size_t f_begin, size_t f_end, uint64_t *d_rows, void *stream) try {
    int rc = check_level_call(ctx, prog, d_wires, T, s_begin, s_count);
    if (rc != FBS_OK) return rc;
    if (level >= prog->depth) return set_error(ctx, FBS_E_INVALID, "level out of range");
    const BootStage &b = prog->boot[level];
    if (f_begin > f_end || f_end > (size_t)b.n_gates * s_count) return set_error(ctx, FBS_E_INVALID, "bad bootstrap range");
    if (f_begin == f_end) return FBS_OK;   // (covers s_count == 0)
    // A level with shared rotations: into the wire slots it runs whole (the tables of one source are cut from one accumulator
    // right after the rotations).  Into rows it can be SLICED: rows are then (k + 1) N words (fbs_layout.row_words), an ordinary gate
    // leaves its ciphertext in its row and a shared rotation its whole accumulator -- the unit dealt out across GPUs is the
    // rotation -- and fbs_level_scatter_dev cuts the tables out once every row is there.
    if (b.n_shared && !d_rows && (f_begin != 0 || f_end != (size_t)b.n_gates * s_count))
        return set_error(ctx, FBS_E_INVALID, "a level of a fused program runs whole when it writes to the wire slots (slice it into rows)");
    GateView gv = level_view(ctx, prog, b, d_wires, d_rows, T, s_begin, s_count, f_begin, f_end);
    rc = ensure_ms(ctx, gv.ks_count);
    if (rc != FBS_OK) return rc;
    if (b.n_shared && !d_rows) {
        if ((rc = ensure_acc(ctx, (size_t)b.n_shared * s_count)) != FBS_OK) return rc;
        gv.acc_rows = ctx->d_acc;
    }
    hipStream_t s = pick(ctx, stream);
    return scratch_section(ctx, s, [&]() -> int {
        if (int rc = dev_keyswitch(ctx, gv, ctx->d_ms, ctx->p.log_n_poly + 1, s)) return rc;
        if (int rc = dev_blind_rotate(ctx, prog->tv, gv, ctx->d_ms, s)) return rc;
        if (!b.n_shared || d_rows) return FBS_OK;
        return dev_multi_extract(ctx, prog->tv, ctx->d_acc, d_wires, T, s_begin, s_count, b.n_extract, b.d_x_row, b.d_x_table, b.d_x_dst, s);
    });
} FBS_API_CATCH(ctx)

int fbs_level_scatter_dev(fbs_ctx *ctx, const fbs_prog *prog, uint32_t level, uint64_t *d_wires, size_t T, size_t s_begin,
                          size_t s_count, const uint64_t *d_rows, size_t f_begin, size_t f_end, void *stream) try {
    int rc = check_level_call(ctx, prog, d_wires, T, s_begin, s_count);
    if (rc != FBS_OK) return rc;
    if (level >= prog->depth) return set_error(ctx, FBS_E_INVALID, "level out of range");
    const BootStage &b = prog->boot[level];
    if (!d_rows || f_begin > f_end || f_end > (size_t)b.n_gates * s_count) return set_error(ctx, FBS_E_INVALID, "bad row range");
    if (!prog->fused) return dev_scatter_rows(ctx, d_wires, T, s_begin, s_count, b.d_dst, d_rows, f_begin, f_end - f_begin, 0, pick(ctx, stream));
    // fused: rows of (k + 1) N words; the tables of shared rotations are cut out of the gathered accumulators, which takes every row
    if (b.n_shared && (f_begin != 0 || f_end != (size_t)b.n_gates * s_count))
        return set_error(ctx, FBS_E_INVALID, "scattering a level of a fused program takes all of its rows");
    rc = dev_scatter_rows(ctx, d_wires, T, s_begin, s_count, b.d_dst, d_rows, f_begin, f_end - f_begin, (ctx->p.k + 1) * ctx->N, pick(ctx, stream));
    if (rc != FBS_OK || !b.n_shared) return rc;
    return dev_multi_extract(ctx, prog->tv, d_rows, d_wires, T, s_begin, s_count, b.n_extract, b.d_x_gate, b.d_x_table, b.d_x_dst,
                             pick(ctx, stream));
} FBS_API_CATCH(ctx)

// ---- audited evaluation (include/fbs_exec.h): the rows of a point, and their exact error statistics -------------------------------
// FBS_OK and the rows of (level, point): their count, wire ids (null for the inputs: wire i) and device slots; or FBS_E_INVALID
static int audit_rows_of(const fbs_prog *prog, uint32_t level, uint32_t point, uint32_t *n_rows, const uint32_t **wire, const uint32_t **d_slot) {
    *wire = nullptr;
    *d_slot = nullptr;
    switch (point) {
    case FBS_AUDIT_INPUTS:
        *n_rows = prog->n_inputs;
        *d_slot = prog->d_in_slot;
        return FBS_OK;
    case FBS_AUDIT_LINCOMB:
        if (level > prog->depth) return FBS_E_INVALID;
        *n_rows = (uint32_t)prog->audit_lin[level].wire.size();
        *wire = prog->audit_lin[level].wire.data();
        *d_slot = prog->audit_lin[level].d_slot;
        return FBS_OK;
    case FBS_AUDIT_ROTATION_INPUT:
        if (level >= prog->depth) return FBS_E_INVALID;
        *n_rows = (uint32_t)prog->audit_src[level].size();
        *wire = prog->audit_src[level].data();
        *d_slot = prog->boot[level].d_src_slot;
        return FBS_OK;
    case FBS_AUDIT_BOOTSTRAP:
        if (level >= prog->depth) return FBS_E_INVALID;
        *n_rows = (uint32_t)prog->audit_boot[level].wire.size();
        *wire = prog->audit_boot[level].wire.data();
        *d_slot = prog->audit_boot[level].d_slot;
        return FBS_OK;
    default:
        return FBS_E_INVALID;
    }
}

int fbs_audit_rows(const fbs_prog *prog, uint32_t level, uint32_t point, uint32_t *n_rows, uint32_t *wire_ids) try {
    if (!prog || !n_rows) return FBS_E_INVALID;
    const uint32_t *wire, *d_slot;
    if (audit_rows_of(prog, level, point, n_rows, &wire, &d_slot) != FBS_OK)
        return set_error(prog->ctx, FBS_E_INVALID, "no such level or point to audit");
    if (wire_ids)
        for (uint32_t r = 0; r < *n_rows; r++) wire_ids[r] = wire ? wire[r] : r;
    return FBS_OK;
} FBS_API_CATCH(prog ? prog->ctx : nullptr)

int fbs_audit_level_dev(fbs_ctx *ctx, const fbs_prog *prog, uint32_t level, uint32_t point, const uint64_t *d_wires, size_t T,
                        size_t s_begin, size_t s_count, const int64_t *d_expected, fbs_audit_row *stats, int64_t *errors, void *stream) try {
    int rc = check_prog(ctx, prog);
    if (rc != FBS_OK) return rc;
    if (ctx->eval_only) return set_error(ctx, FBS_E_STATE, EVAL_ONLY);
    uint32_t n_rows = 0;
    const uint32_t *wire, *d_slot;
    if (audit_rows_of(prog, level, point, &n_rows, &wire, &d_slot) != FBS_OK)
        return set_error(ctx, FBS_E_INVALID, "no such level or point to audit");
    if (s_begin > T || s_count > T - s_begin) return set_error(ctx, FBS_E_INVALID, "bad sample range");
    if (n_rows == 0 || s_count == 0) return FBS_OK;
    if (!d_wires || !d_expected || !stats) return set_error(ctx, FBS_E_INVALID, "null argument");
    // the bound under which the reduction's 64-bit sum and 128-bit sum of squares cannot overflow (fbs_audit.hip)
    if (s_count > AUDIT_MAX_SAMPLES) return set_error(ctx, FBS_E_INVALID, "more than 2^18 samples in one audit call");
    const size_t total = (size_t)n_rows * s_count;
    const bool fields = point == FBS_AUDIT_ROTATION_INPUT;
    if ((rc = ensure_audit(ctx, n_rows, total)) != FBS_OK) return rc;
    if (fields && (rc = ensure_ms(ctx, total)) != FBS_OK) return rc;
    hipStream_t s = pick(ctx, stream);
    rc = scratch_section(ctx, s, [&]() -> int {
        int rc;
        if (fields) {
            // the key switch of fbs_level_bootstrap_dev(level) over the level's full range: the same view, the same width, the same scratch
            const BootStage &b = prog->boot[level];
            const GateView gv = level_view(ctx, prog, b, const_cast<uint64_t *>(d_wires), nullptr, T, s_begin, s_count, 0, (size_t)b.n_gates * s_count);
            if ((rc = dev_keyswitch(ctx, gv, ctx->d_ms, ctx->p.log_n_poly + 1, s)) != FBS_OK) return rc;
            rc = dev_audit_fields(ctx, ctx->d_ms, n_rows, s_count, d_expected, ctx->d_audit_err, s);
        } else {
            rc = dev_audit_wire(ctx, d_wires, d_slot, n_rows, T, s_begin, s_count, d_expected, ctx->d_audit_err, s);
        }
        if (rc != FBS_OK || (rc = dev_audit_reduce(ctx, ctx->d_audit_err, n_rows, s_count, fields, ctx->d_audit_stats, s)) != FBS_OK) return rc;
        if (hipMemcpyAsync(stats, ctx->d_audit_stats, (size_t)n_rows * sizeof(fbs_audit_row), hipMemcpyDeviceToHost, s) != hipSuccess ||
            (errors && hipMemcpyAsync(errors, ctx->d_audit_err, total * 8, hipMemcpyDeviceToHost, s) != hipSuccess))
            return set_error(ctx, FBS_E_DEVICE, "copying the audit's results back failed");
        return FBS_OK;
    });
    if (rc != FBS_OK) return rc;
    FBS_HIP(ctx, hipStreamSynchronize(s));
    return FBS_OK;
} FBS_API_CATCH(ctx)

// ---- compact outputs: their decryption (fbs_compact_dev and the compact store stage: fbs_eval.cpp) ------------------------------
int fbs_decrypt_compact_dev(const fbs_ctx *ctx, const uint64_t *d_words, size_t count, uint32_t bits, int64_t *d_msgs, void *stream) try {
    if (int rc = io_prologue(ctx, d_words, d_msgs, count, IO_SECRET, nullptr)) return rc;
    if (int rc = check_bits(ctx, bits)) return rc;
    if (int rc = check_compact_words(ctx, count, bits)) return rc;
    if (count == 0) return FBS_OK;
    FBS_HIP(ctx, hipSetDevice(ctx->device));
    return dev_decrypt_compact(ctx, d_words, count, bits, d_msgs, pick(ctx, stream));
} FBS_API_CATCH(ctx)

// ---- chained evaluation: compact ciphertexts back into the blind rotation (programs over mixed sources: fbs_eval.cpp) -----------
// (no secret needed; no scratch: the fields go straight to the caller's buffer)
int fbs_compact_fields_dev(fbs_ctx *ctx, const uint64_t *d_words, size_t count, uint32_t bits, uint32_t *d_fields, void *stream) try {
    if (int rc = io_prologue(ctx, d_words, d_fields, count, 0, nullptr)) return rc;
    if (int rc = check_bits(ctx, bits)) return rc;
    if (int rc = check_compact_words(ctx, count, bits)) return rc;
    if (count > SIZE_MAX / 4 / (ctx->p.n + 1)) return set_error(ctx, FBS_E_INVALID, "count * (n + 1) fields overflow");
    if (count == 0) return FBS_OK;
    FBS_HIP(ctx, hipSetDevice(ctx->device));
    return dev_compact_unpack(ctx, d_words, count, bits, d_fields, pick(ctx, stream));
} FBS_API_CATCH(ctx)

// unpack into the modulus-switch scratch, then one blind rotation through the identity table: in passes like fbs_compact_dev
int fbs_refresh_compact_dev(fbs_ctx *ctx, const uint64_t *d_words, size_t count, uint32_t bits, uint64_t *d_cts, void *stream) try {
    if (int rc = io_prologue(ctx, d_words, d_cts, count, IO_CT_WORDS, nullptr)) return rc;
    if (int rc = check_bits(ctx, bits)) return rc;
    if (int rc = check_compact_words(ctx, count, bits)) return rc;
    if (count == 0) return FBS_OK;
    FBS_HIP(ctx, hipSetDevice(ctx->device));
    fbs_tvset *tv = nullptr;
    int rc = identity_tv(ctx, &tv);
    if (rc != FBS_OK) return rc;
    const size_t ctw = ctx->D + 1, W = compact_words(ctx->p.n, bits);
    hipStream_t s = pick(ctx, stream);
    return ms_passes(ctx, count, s, [&](size_t f0, size_t rows) {
        if (int rc = dev_compact_unpack(ctx, d_words + f0 * W, rows, bits, ctx->d_ms, s)) return rc;
        return dev_blind_rotate(ctx, tv, batch_view(nullptr, d_cts + f0 * ctw, nullptr, rows), ctx->d_ms, s);
    });
} FBS_API_CATCH(ctx)

// ---- resident state: device blocks of ciphertexts that stay on the card between evaluations (fbs_state.hip) -----------------
int fbs_state_create(fbs_ctx *ctx, size_t rows, size_t T, fbs_state **out) try {
    if (!ctx || !out) return FBS_E_INVALID;
    *out = nullptr;
    if (rows == 0 || T == 0) return set_error(ctx, FBS_E_INVALID, "a state has at least one row and one sample");
    if (rows > FBS_MAX_WIRES) return set_error(ctx, FBS_E_INVALID, "state too large: rows exceed FBS_MAX_WIRES");
    if (T > SIZE_MAX / 8 / rows / (ctx->D + 1)) return set_error(ctx, FBS_E_INVALID, "rows * T * (D + 1) words overflow");
    FBS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t bytes = rows * T * (ctx->D + 1) * 8;
    std::unique_ptr<fbs_state> st(new fbs_state);
    ctx->states.reserve(ctx->states.size() + 1);
    const hipError_t e = hipMalloc(&st->d, bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();   // (an allocation that fails leaves the device, and so the context, as it was)
        return set_error(ctx, FBS_E_DEVICE, "a state of " + std::to_string(bytes) + " bytes: " + hipGetErrorString(e));
    }
    st->ctx = ctx;
    st->rows = rows;
    st->T = T;
    ctx->states.push_back(st.get());
    ctx->state_bytes += bytes;
    *out = st.release();
    return FBS_OK;
} FBS_API_CATCH(ctx)

void fbs_state_destroy(fbs_state *st) try {
    if (!st) return;
    fbs_ctx *ctx = st->ctx;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);   // queued evaluations may still read or write it
    if (ctx->scratch_used) (void)hipStreamSynchronize(ctx->scratch_stream);
    ctx->states.erase(std::remove(ctx->states.begin(), ctx->states.end(), st), ctx->states.end());
    ctx->state_bytes -= st->rows * st->T * (ctx->D + 1) * 8;
    (void)hipFree(st->d);
    delete st;
} catch (...) {
}

int fbs_state_info(const fbs_state *st, size_t *rows, size_t *T) try {
    if (!st) return FBS_E_INVALID;
    if (rows) *rows = st->rows;
    if (T) *T = st->T;
    return FBS_OK;
} FBS_API_CATCH(st ? st->ctx : nullptr)

// what fetch and put check: the state is this context's, the rows are its rows
static int check_state_rows(const fbs_ctx *ctx, const fbs_state *st, size_t row0, size_t rows, const void *host) {
    if (!state_of(ctx, st)) return set_error(ctx, FBS_E_INVALID, "not a live state of this context");
    if (row0 > st->rows || rows > st->rows - row0) return set_error(ctx, FBS_E_INVALID, "rows past the end of the state");
    if (rows && !host) return set_error(ctx, FBS_E_INVALID, "null argument");
    return FBS_OK;
}
// rows [row0, row0 + rows) of a checked state, flattened [row][sample]: one run of rows * T ciphertexts, which the kernels read and
// write as they do a plain batch (a state's rows * T * (D + 1) words fit a size_t)
struct StateSpan {
    uint64_t *d;
    size_t count;
};
static StateSpan state_span(const fbs_ctx *ctx, const fbs_state *st, size_t row0, size_t rows) {
    return {st->d + row0 * st->T * (ctx->D + 1), rows * st->T};
}

int fbs_state_fetch(fbs_ctx *ctx, const fbs_state *st, size_t row0, size_t rows, uint32_t bits, uint64_t *out) try {
    if (!ctx) return FBS_E_INVALID;
    int rc = check_state_rows(ctx, st, row0, rows, out);
    if (rc != FBS_OK) return rc;
    if (bits && (rc = check_bits(ctx, bits)) != FBS_OK) return rc;
    if (rows == 0) return FBS_OK;
    FBS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const StateSpan span = state_span(ctx, st, row0, rows);
    const size_t ctw = ctx->D + 1, count = span.count;
    const uint64_t *d_cts = span.d;
    if (!bits) {
        FBS_HIP(ctx, hipMemcpyAsync(out, d_cts, count * ctw * 8, hipMemcpyDeviceToHost, s));
        return sync_stream(ctx, s);
    }
    if (!ctx->have_keys) return set_error(ctx, FBS_E_STATE, "fbs_keygen has not run");
    // fbs_compact_dev's passes, each packed into the staging of the compact outputs and copied back from there
    const size_t W = compact_words(ctx->p.n, bits);
    if ((rc = grow(ctx, ctx->d_compact, ctx->compact_capacity, ms_pass_size(ctx, count) * W, 8, true)) != FBS_OK) return rc;
    rc = ms_passes(ctx, count, s, [&](size_t f0, size_t n) {
        const GateView gv = batch_view(d_cts + f0 * ctw, nullptr, nullptr, n);
        if (int rc = dev_keyswitch(ctx, gv, ctx->d_ms, bits, s)) return rc;
        if (int rc = dev_compact_pack(ctx, ctx->d_ms, n, bits, ctx->d_compact, s)) return rc;
        if (hipMemcpyAsync(out + f0 * W, ctx->d_compact, n * W * 8, hipMemcpyDeviceToHost, s) != hipSuccess)
            return set_error(ctx, FBS_E_DEVICE, "copying compact words to the host failed");
        return FBS_OK;
    });
    return rc != FBS_OK ? rc : sync_stream(ctx, s);
} FBS_API_CATCH(ctx)

int fbs_state_put(fbs_ctx *ctx, fbs_state *st, size_t row0, size_t rows, const uint64_t *cts) try {
    if (!ctx) return FBS_E_INVALID;
    if (int rc = check_state_rows(ctx, st, row0, rows, cts)) return rc;
    if (rows == 0) return FBS_OK;
    const StateSpan span = state_span(ctx, st, row0, rows);
    const size_t words = span.count * (ctx->D + 1);
    for (size_t i = 0; i < words; i++)
        if (cts[i] >= FQ) return set_error(ctx, FBS_E_INVALID, "word " + std::to_string(i) + " is not a canonical residue");
    FBS_HIP(ctx, hipSetDevice(ctx->device));
    FBS_HIP(ctx, hipMemcpyAsync(span.d, cts, words * 8, hipMemcpyHostToDevice, ctx->stream));
    return sync_stream(ctx, ctx->stream);
} FBS_API_CATCH(ctx)

// ---- sample-axis operations: the group sum (fbs_state.hip); the mapped evaluation is fbs_eval.cpp's ---------------------------
int fbs_state_sum_groups(fbs_ctx *ctx, const fbs_state *src, size_t row0, size_t rows, size_t group, fbs_state *dst, size_t dst_row0) try {
    if (!ctx) return FBS_E_INVALID;
    if (!state_of(ctx, src) || !state_of(ctx, dst)) return set_error(ctx, FBS_E_INVALID, "not a live state of this context");
    if (src == dst) return set_error(ctx, FBS_E_INVALID, "the sums of a state do not go into the same state");
    if (group < 1 || group > FBS_MAX_SUM_GROUP) return set_error(ctx, FBS_E_INVALID, "group " + std::to_string(group) + " outside [1, 65536]");
    if (row0 > src->rows || rows > src->rows - row0 || dst_row0 > dst->rows || rows > dst->rows - dst_row0)
        return set_error(ctx, FBS_E_INVALID, "rows past the end of the state");
    const size_t T_dst = (src->T - 1) / group + 1;
    if (dst->T != T_dst)
        return set_error(ctx, FBS_E_INVALID, "the destination holds " + std::to_string(dst->T) + " samples a row, groups of " + std::to_string(group) +
                                                 " of " + std::to_string(src->T) + " samples make " + std::to_string(T_dst));
    if (rows == 0) return FBS_OK;
    FBS_HIP(ctx, hipSetDevice(ctx->device));
    return dev_state_sum_groups(ctx, SumGroups{state_span(ctx, src, row0, rows).d, state_span(ctx, dst, dst_row0, rows).d, rows, src->T, T_dst, group, ctx->D},
                                ctx->stream);
} FBS_API_CATCH(ctx)

// ---- public-key inputs: the device side of the expansion (fbs_public.hip); the host entries are fbs_public.cpp's ---------------
int fbs_pub_expand_dev(fbs_ctx *ctx, const uint64_t *d_glwe, size_t count, uint64_t *d_cts, void *stream) try {
    if (!ctx || (count && (!d_glwe || !d_cts))) return FBS_E_INVALID;
    if (int rc = check_ct_words(ctx, count)) return rc;
    if (count == 0) return FBS_OK;
    FBS_HIP(ctx, hipSetDevice(ctx->device));
    return dev_expand_public(ctx, d_glwe, count, d_cts, pick(ctx, stream));
} FBS_API_CATCH(ctx)

int fbs_state_put_public(fbs_ctx *ctx, fbs_state *st, size_t row0, size_t rows, const uint64_t *glwe) try {
    if (!ctx) return FBS_E_INVALID;
    int rc = check_state_rows(ctx, st, row0, rows, glwe);
    if (rc != FBS_OK) return rc;
    if (rows == 0) return FBS_OK;
    const StateSpan span = state_span(ctx, st, row0, rows);
    const size_t count = span.count, words = (count + ctx->N - 1) / ctx->N * ((size_t)ctx->D + ctx->N);   // (the samples are fewer words)
    const size_t bad = first_noncanonical(glwe, words);
    if (bad < words) return set_error(ctx, FBS_E_INVALID, "sample word " + std::to_string(bad) + " is not a canonical residue");
    FBS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    if ((rc = grow(ctx, ctx->d_pub, ctx->pub_capacity, words, 8, true)) != FBS_OK) return rc;
    rc = scratch_section(ctx, s, [&]() -> int {
        if (hipMemcpyAsync(ctx->d_pub, glwe, words * 8, hipMemcpyHostToDevice, s) != hipSuccess)
            return set_error(ctx, FBS_E_DEVICE, "copying samples to the device failed");
        return dev_expand_public(ctx, ctx->d_pub, count, span.d, s);
    });
    return rc != FBS_OK ? rc : sync_stream(ctx, s);
} FBS_API_CATCH(ctx)

// ---- the gadget keys (GadgetKind, fbs_internal.hpp): the packing key of packed outputs, the fold key of folded state ------------
// installs (t, gamma, bodies) as the context's key of `kind`: expands the masks, transforms on the device; the previous key stays
// until this has succeeded
static int install_gadget_key(fbs_ctx *ctx, GadgetKind kind, uint32_t t, uint32_t gamma, std::vector<uint64_t> &bodies) {
    HostState::GadgetKeyState &key = ctx->gadget[kind];
    std::vector<uint64_t> full;
    host_expand_gadget_key(ctx, kind, ctx->mask_key, t, bodies.data(), full);
    const bool had = key.have;
    key.have = false;
    if (int rc = dev_upload_gadget_key(ctx, kind, full, t)) {
        // (the device copy may be half written: re-install the previous key, or leave the context without one)
        if (had) {
            host_expand_gadget_key(ctx, kind, ctx->mask_key, key.t, key.bodies.data(), full);
            const std::string text = ctx->err;
            key.have = dev_upload_gadget_key(ctx, kind, full, key.t) == FBS_OK;
            ctx->err = text;
        }
        return rc;
    }
    gadget_key_in_place(ctx, kind, t, gamma, bodies);
    return FBS_OK;
}
static int gadget_keygen(fbs_ctx *ctx, GadgetKind kind, uint32_t t, uint32_t gamma) {
    if (int rc = check_gadget_keygen(ctx, kind, t, gamma)) return rc;
    FBS_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<uint64_t> bodies;
    if (ctx->tune.keys_on_device) {
        if (int rc = dev_gadget_bodies(ctx, kind, t, gamma, bodies)) return rc;
    } else {
        host_gadget_keygen(ctx, kind, t, gamma, bodies);
    }
    return install_gadget_key(ctx, kind, t, gamma, bodies);
}
// (no secret needed: the masks come from the mask key an evaluation-only context has received)
static int import_gadget_key(fbs_ctx *ctx, GadgetKind kind, uint32_t t, uint32_t gamma, const uint64_t *bodies) {
    if (!ctx) return FBS_E_INVALID;
    if (!bodies) return set_error(ctx, FBS_E_INVALID, "null argument");
    if (int rc = check_gadget_keygen(ctx, kind, t, gamma, false, "fbs_import_seeded_keys")) return rc;
    const size_t words = (size_t)gadget_rows(*ctx, kind) * t * ctx->N;
    for (size_t i = 0; i < words; i++)
        if (bodies[i] >= FQ) return set_error(ctx, FBS_E_INVALID, gadget_text(kind, "@-key body word is not a canonical residue"));
    FBS_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<uint64_t> copy(bodies, bodies + words);
    return install_gadget_key(ctx, kind, t, gamma, copy);
}

int fbs_packing_keygen(fbs_ctx *ctx, uint32_t t_p, uint32_t gamma_p) try {
    return gadget_keygen(ctx, GK_PACK, t_p, gamma_p);
} FBS_API_CATCH(ctx)

int fbs_import_packing_key(fbs_ctx *ctx, uint32_t t_p, uint32_t gamma_p, const uint64_t *bodies) try {
    return import_gadget_key(ctx, GK_PACK, t_p, gamma_p, bodies);
} FBS_API_CATCH(ctx)

int fbs_fold_keygen(fbs_ctx *ctx, uint32_t t_f, uint32_t gamma_f) try {
    return gadget_keygen(ctx, GK_FOLD, t_f, gamma_f);
} FBS_API_CATCH(ctx)

int fbs_fold_key_sizes(const fbs_ctx *ctx, uint32_t t_f, size_t sizes[2]) try {
    return gadget_key_sizes(ctx, GK_FOLD, t_f, sizes);
} FBS_API_CATCH(ctx)

int fbs_export_fold_key(const fbs_ctx *ctx, uint64_t *bodies, uint64_t *full) try {
    return gadget_key_export(ctx, GK_FOLD, bodies, full);
} FBS_API_CATCH(ctx)

int fbs_import_fold_key(fbs_ctx *ctx, uint32_t t_f, uint32_t gamma_f, const uint64_t *bodies) try {
    return import_gadget_key(ctx, GK_FOLD, t_f, gamma_f, bodies);
} FBS_API_CATCH(ctx)

// ---- packed outputs: up to N outputs in one GLWE sample under the big key (fbs_pack.hpp, fbs_pack.hip); folded state: N resident
// ---- ciphertexts in one full-precision GLWE sample under the big key (fbs_fold.hip) ------------------------------------------------
// what both check first; the words of the result must not overflow (folding: the samples are fewer words than the ciphertexts)
static int gadget_prologue(const fbs_ctx *ctx, GadgetKind kind, size_t count, uint32_t bits) {
    if (!ctx->have_keys) return set_error(ctx, FBS_E_STATE, "fbs_keygen has not run");
    if (!ctx->gadget[kind].have) return set_error(ctx, FBS_E_STATE, gadget_text(kind, "the context has no @ key (fbs_@_keygen / fbs_import_@_key)"));
    if (kind == GK_FOLD) return check_ct_words(ctx, count);
    if (int rc = check_bits(ctx, bits)) return rc;
    return check_packed_words(ctx, count, bits);
}
// The scratch both share for a pass of `pass` ciphertexts, grown like any other: `col_words` field words a ciphertext, and the
// partial accumulators of a sum over `rows` key rows
static int pack_scratch_reserve(fbs_ctx *ctx, size_t pass, size_t col_words, uint32_t rows) {
    if (int rc = grow(ctx, ctx->d_pack_fields, ctx->pack_fields_capacity, col_words * pass, 4, true)) return rc;
    // (slices x samples is largest for the whole pass or for a single sample, whichever the launch rule favours)
    size_t acc = 0;
    for (size_t g = 1; g <= pass / ctx->N; g++) acc = std::max(acc, g * pack_slices_for(ctx, g, rows));
    return grow(ctx, ctx->d_pack_acc, ctx->pack_acc_capacity, acc * (ctx->p.k + 1) * ctx->N, 8, true);
}
// Ciphertexts per pass: what the modulus-switch scratch holds (at least COMPACT_PASS), cut down to whole samples -- and the
// scratch for a pass of that size: the modulus switch's, the transposed fields [n + 1]
static int pack_reserve(fbs_ctx *ctx, size_t count, size_t *pass_out) {
    const size_t N = ctx->N, whole = std::max(ctx->ms_capacity, COMPACT_PASS) / N * N;
    *pass_out = std::min((count + N - 1) / N * N, whole);
    if (int rc = ensure_ms(ctx, std::min(count, *pass_out))) return rc;
    return pack_scratch_reserve(ctx, *pass_out, (size_t)ctx->p.n + 1, ctx->p.n);
}
// Ciphertexts per pass: COMPACT_PASS cut down to whole samples (one sample at N = 4096 and above it) -- and the scratch for a pass
// of that size: D rows of rounded fields and the 64-bit body words
static int fold_reserve(fbs_ctx *ctx, size_t count, size_t *pass_out) {
    const size_t N = ctx->N, whole = std::max(COMPACT_PASS, N) / N * N;
    *pass_out = std::min((count + N - 1) / N * N, whole);
    return pack_scratch_reserve(ctx, *pass_out, (size_t)ctx->D + 2, ctx->D);
}
// What the five entries below do once their arguments are checked: the scratch, then inside one scratch section the passes of
// `count` ciphertexts at d_cts, packed at `bits` (GK_PACK) or folded (GK_FOLD).  A pass of `rows` ciphertexts leaves words_of(rows)
// words, in d_dst at words_of(pass) a pass -- or, `out` given, in the kind's staging and from there in that host array, which is
// complete when the call returns.  d_map (a mapped fold): position j takes ciphertext d_map[j] of the n_src at d_cts
static int gadget_passes(fbs_ctx *ctx, GadgetKind kind, const uint64_t *d_cts, size_t count, uint32_t bits, uint64_t *d_dst, uint64_t *out,
                         hipStream_t s, const uint32_t *d_map = nullptr, size_t n_src = 0) {
    FBS_HIP(ctx, hipSetDevice(ctx->device));
    const uint32_t N = ctx->N, k = ctx->p.k;
    const bool packing = kind == GK_PACK;
    size_t pass = 0;
    int rc = packing ? pack_reserve(ctx, count, &pass) : fold_reserve(ctx, count, &pass);
    if (rc != FBS_OK) return rc;
    auto words_of = [=](size_t rows) { return packing ? packed_words(k, N, rows, bits) : (rows + N - 1) / N * ((size_t)k * N + N); };
    if (out) {
        fbs_ctx::GadgetKeyDev &dev = ctx->gadget_dev[kind];
        if ((rc = grow(ctx, dev.d_out, dev.out_capacity, words_of(pass), 8, true)) != FBS_OK) return rc;
        d_dst = dev.d_out;
    }
    rc = scratch_section(ctx, s, [&]() -> int {
        const size_t ctw = ctx->D + 1;
        for (size_t f0 = 0; f0 < count; f0 += pass) {
            const size_t rows = std::min(pass, count - f0), w0 = f0 / pass * words_of(pass);
            const uint64_t *cts = d_map ? d_cts : d_cts + f0 * ctw;
            uint64_t *dst = out ? d_dst : d_dst + w0;
            int rc = packing ? dev_keyswitch(ctx, batch_view(cts, nullptr, nullptr, rows), ctx->d_ms, 31, s)
                             : dev_fold(ctx, cts, rows, dst, s, d_map ? d_map + f0 : nullptr, n_src);
            if (rc == FBS_OK && packing) rc = dev_pack(ctx, ctx->d_ms, rows, bits, dst, s);
            if (rc != FBS_OK) return rc;
            if (out && hipMemcpyAsync(out + w0, dst, words_of(rows) * 8, hipMemcpyDeviceToHost, s) != hipSuccess)
                return set_error(ctx, FBS_E_DEVICE, packing ? "copying packed words to the host failed" : "copying folded samples to the host failed");
        }
        return FBS_OK;
    });
    return rc != FBS_OK || !out ? rc : sync_stream(ctx, s);
}

// (no secret needed: runs on evaluation-only contexts)
int fbs_pack_dev(fbs_ctx *ctx, const uint64_t *d_cts, size_t count, uint32_t bits, uint64_t *d_words, void *stream) try {
    if (int rc = io_prologue(ctx, d_cts, d_words, count, IO_CT_WORDS, nullptr)) return rc;
    if (int rc = gadget_prologue(ctx, GK_PACK, count, bits)) return rc;
    if (count == 0) return FBS_OK;
    return gadget_passes(ctx, GK_PACK, d_cts, count, bits, d_words, nullptr, pick(ctx, stream));
} FBS_API_CATCH(ctx)

int fbs_state_fetch_packed(fbs_ctx *ctx, const fbs_state *st, size_t row0, size_t rows, uint32_t bits, uint64_t *out) try {
    if (!ctx) return FBS_E_INVALID;
    if (int rc = check_state_rows(ctx, st, row0, rows, out)) return rc;
    const StateSpan span = state_span(ctx, st, row0, rows);
    if (int rc = gadget_prologue(ctx, GK_PACK, span.count, bits)) return rc;
    if (rows == 0) return FBS_OK;
    return gadget_passes(ctx, GK_PACK, span.d, span.count, bits, nullptr, out, ctx->stream);
} FBS_API_CATCH(ctx)

// folded samples are written 16 bytes a lane
static int check_fold_target(const fbs_ctx *ctx, const uint64_t *d_glwe) {
    if ((uintptr_t)d_glwe & 15u) return set_error(ctx, FBS_E_INVALID, "folded samples are written 16 bytes a lane: d_glwe must be 16-byte aligned");
    return FBS_OK;
}

// (no secret needed: runs on evaluation-only contexts)
int fbs_fold_dev(fbs_ctx *ctx, const uint64_t *d_cts, size_t count, uint64_t *d_glwe, void *stream) try {
    if (!ctx || (count && (!d_cts || !d_glwe))) return FBS_E_INVALID;
    if (int rc = gadget_prologue(ctx, GK_FOLD, count, 0)) return rc;
    if (int rc = check_fold_target(ctx, d_glwe)) return rc;
    if (count == 0) return FBS_OK;
    return gadget_passes(ctx, GK_FOLD, d_cts, count, 0, d_glwe, nullptr, pick(ctx, stream));
} FBS_API_CATCH(ctx)

// ---- encrypted-index reads (include/fbs_exec.h): the mapped fold that lays a table out, the rotation that reads it ----------------
int fbs_lookup_map(uint32_t p, uint32_t N, uint32_t len, uint32_t base, uint32_t stride, uint32_t *map_out) try {
    return host_lookup_map(p, N, len, base, stride, map_out);
} FBS_API_CATCH(nullptr)

// (no secret needed: runs on evaluation-only contexts)
int fbs_fold_mapped_dev(fbs_ctx *ctx, const uint64_t *d_cts, size_t n_src, const uint32_t *d_map, size_t count, uint64_t *d_glwe,
                        void *stream) try {
    if (!ctx || (count && (!d_cts || !d_map || !d_glwe))) return FBS_E_INVALID;
    if (int rc = gadget_prologue(ctx, GK_FOLD, count, 0)) return rc;
    if (int rc = check_ct_words(ctx, n_src)) return rc;
    if (int rc = check_fold_target(ctx, d_glwe)) return rc;
    if (count == 0) return FBS_OK;
    if (n_src == 0 || n_src >= FOLD_MAP_NEG) return set_error(ctx, FBS_E_INVALID, "a mapped fold reads 1 .. 2^31 - 1 source ciphertexts");
    return gadget_passes(ctx, GK_FOLD, d_cts, count, 0, d_glwe, nullptr, pick(ctx, stream), d_map, n_src);
} FBS_API_CATCH(ctx)

// what both lookups check once their buffers and keys are: the tables
static int check_lookup_tables(const fbs_ctx *ctx, const uint64_t *d_tables, uint32_t n_tables, size_t count) {
    if (count && (!d_tables || n_tables == 0)) return set_error(ctx, FBS_E_INVALID, "a lookup needs at least one table");
    if ((uintptr_t)d_tables & 15u) return set_error(ctx, FBS_E_INVALID, "tables are folded samples: d_tables must be 16-byte aligned");
    if (count > 0x7FFFFFFFull) return set_error(ctx, FBS_E_INVALID, "batch too large");
    return FBS_OK;
}

// (needs neither a secret nor a fold key)
int fbs_lookup_dev(fbs_ctx *ctx, const uint64_t *d_tables, uint32_t n_tables, const uint32_t *d_table_of, const uint64_t *d_cts_index,
                   size_t count, uint64_t *d_cts_out, void *stream) try {
    if (int rc = io_prologue(ctx, d_cts_index, d_cts_out, count, IO_CT_WORDS, nullptr)) return rc;
    if (int rc = check_lookup_tables(ctx, d_tables, n_tables, count)) return rc;
    if (count == 0) return FBS_OK;
    FBS_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = ensure_ms(ctx, count)) return rc;
    const GateView gv = batch_view(d_cts_index, d_cts_out, nullptr, count);
    const BrStart start{d_tables, n_tables, d_table_of, 0};
    hipStream_t s = pick(ctx, stream);
    return scratch_section(ctx, s, [&]() -> int {
        if (int rc = dev_keyswitch(ctx, gv, ctx->d_ms, ctx->p.log_n_poly + 1, s)) return rc;
        return dev_blind_rotate(ctx, nullptr, gv, ctx->d_ms, s, &start);
    });
} FBS_API_CATCH(ctx)

// fbs_refresh_compact_dev with the table in place of the identity polynomial: its passes, its unpack
int fbs_lookup_compact_dev(fbs_ctx *ctx, const uint64_t *d_tables, uint32_t n_tables, const uint32_t *d_table_of, const uint64_t *d_words,
                           size_t count, uint32_t bits, uint64_t *d_cts_out, void *stream) try {
    if (int rc = io_prologue(ctx, d_words, d_cts_out, count, IO_CT_WORDS, nullptr)) return rc;
    if (int rc = check_bits(ctx, bits)) return rc;
    if (int rc = check_compact_words(ctx, count, bits)) return rc;
    if (int rc = check_lookup_tables(ctx, d_tables, n_tables, count)) return rc;
    if (count == 0) return FBS_OK;
    FBS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t ctw = ctx->D + 1, W = compact_words(ctx->p.n, bits);
    hipStream_t s = pick(ctx, stream);
    return ms_passes(ctx, count, s, [&](size_t f0, size_t rows) {
        if (int rc = dev_compact_unpack(ctx, d_words + f0 * W, rows, bits, ctx->d_ms, s)) return rc;
        const BrStart start{d_tables, n_tables, d_table_of, f0};
        return dev_blind_rotate(ctx, nullptr, batch_view(nullptr, d_cts_out + f0 * ctw, nullptr, rows), ctx->d_ms, s, &start);
    });
} FBS_API_CATCH(ctx)

// Resident state read by an encrypted index: for every sample s of the index state and every plane m, row out_row0 + m of the output
// at sample s is the entry of plane m's table that index row `index_row` names at sample s.  The maps (the box map per table), the
// table each bootstrap reads and the planes' one shared key-switch source are made on the host and uploaded once; the tables are
// one mapped fold into a scratch of their own; the rotation is one dev_blind_rotate whose planes share the index's key switch and
// modulus switch through GateView::source_of.  Table (m, s) is number m T + s, or m where the planes' tables are shared.
int fbs_state_lookup(fbs_ctx *ctx, const fbs_state *table_state, const uint32_t *rows, uint32_t n_planes, uint32_t len, uint32_t axis,
                     const fbs_state *index_state, size_t index_row, fbs_state *out_state, size_t out_row0) try {
    if (!ctx) return FBS_E_INVALID;
    if (!state_of(ctx, table_state) || !state_of(ctx, index_state) || !state_of(ctx, out_state))
        return set_error(ctx, FBS_E_INVALID, "not a live state of this context");
    if (!rows || n_planes == 0) return set_error(ctx, FBS_E_INVALID, "a lookup reads at least one plane");
    if (axis > 1) return set_error(ctx, FBS_E_INVALID, "axis is 0 (rows) or 1 (samples)");
    if (out_state == table_state || out_state == index_state) return set_error(ctx, FBS_E_INVALID, "the output state must be another state");
    const size_t T = index_state->T, Tt = table_state->T;
    const uint32_t N = ctx->N, p = ctx->p.p_msg, k1 = ctx->p.k + 1;
    if (len == 0) return set_error(ctx, FBS_E_INVALID, "a table has at least one entry");
    if (len > p) return set_error(ctx, FBS_E_INVALID, "a table has at most p entries");
    if (axis == 0 && Tt != 1 && Tt != T) return set_error(ctx, FBS_E_INVALID, "the table state has neither one sample nor the index state's");
    if (axis == 1 && Tt != len) return set_error(ctx, FBS_E_INVALID, "along the samples a table is the table state's samples: len must be its T");
    if (index_row >= index_state->rows) return set_error(ctx, FBS_E_INVALID, "rows past the end of the state");
    if (out_state->T != T || out_row0 > out_state->rows || n_planes > out_state->rows - out_row0)
        return set_error(ctx, FBS_E_INVALID, "the output state holds n_planes rows of the index state's samples from out_row0 on");
    const size_t n_rows = axis == 0 ? (size_t)n_planes * len : n_planes;
    for (size_t i = 0; i < n_rows; i++)
        if (rows[i] >= table_state->rows) return set_error(ctx, FBS_E_INVALID, "rows past the end of the state");
    const bool shared = axis == 1 || Tt == 1;
    const size_t n_tab = shared ? n_planes : (size_t)n_planes * T, n_src = table_state->rows * Tt, count = (size_t)n_planes * T;
    if (n_src >= FOLD_MAP_NEG || n_tab > 0x7FFFFFFFull / N || count > 0x7FFFFFFFull) return set_error(ctx, FBS_E_INVALID, "batch too large");
    if (int rc = gadget_prologue(ctx, GK_FOLD, n_tab * N, 0)) return rc;
    FBS_HIP(ctx, hipSetDevice(ctx->device));
    // the index arrays: [n_tab][N] maps, [count] table of bootstrap f = m T + s, [n_planes] zeros (every plane reads source 0)
    std::vector<uint32_t> idx(n_tab * N + count + n_planes, 0u);
    std::vector<uint32_t> box(N);
    for (uint32_t j = 0; j < N; j++) box[j] = (uint32_t)(((uint64_t)j * 2 * p + N) / (2ull * N));
    for (size_t t = 0; t < n_tab; t++) {
        const size_t m = shared ? t : t / T, s = shared ? 0 : t % T;
        auto src = [&](uint32_t x) -> uint32_t {
            return axis == 0 ? (uint32_t)((size_t)rows[m * len + x] * Tt + (Tt == 1 ? 0 : s)) : (uint32_t)((size_t)rows[m] * Tt + x);
        };
        uint32_t *map = idx.data() + t * N;
        for (uint32_t j = 0; j < N; j++) map[j] = box[j] < len ? src(box[j]) : box[j] < p ? FOLD_MAP_NONE : src(0) | FOLD_MAP_NEG;
    }
    for (size_t f = 0; f < count; f++) idx[n_tab * N + f] = (uint32_t)(shared ? f / T : f);
    hipStream_t s = ctx->stream;
    if (int rc = grow(ctx, ctx->d_lookup_idx, ctx->lookup_idx_capacity, idx.size(), 4, false)) return rc;
    if (int rc = grow(ctx, ctx->d_lookup_tables, ctx->lookup_tables_capacity, n_tab * k1 * N, 8, true)) return rc;
    if (int rc = ensure_ms(ctx, T)) return rc;
    if (ctx->scratch_used) FBS_HIP(ctx, hipStreamSynchronize(ctx->scratch_stream));   // (an earlier call may still read the index arrays)
    FBS_HIP(ctx, hipMemcpy(ctx->d_lookup_idx, idx.data(), idx.size() * 4, hipMemcpyHostToDevice));
    if (int rc = gadget_passes(ctx, GK_FOLD, table_state->d, n_tab * N, 0, ctx->d_lookup_tables, nullptr, s, ctx->d_lookup_idx, n_src)) return rc;
    ctx->lookup_tables = (int64_t)n_tab;
    const size_t ctw = ctx->D + 1;
    GateView gv{};
    gv.in_base = index_state->d + index_row * T * ctw;
    gv.out_base = out_state->d + out_row0 * T * ctw;
    gv.source_of = ctx->d_lookup_idx + n_tab * N + count;
    gv.T = T, gv.s_count = T, gv.count = count, gv.ks_count = T, gv.n_gates = n_planes;
    const BrStart start{ctx->d_lookup_tables, (uint32_t)n_tab, ctx->d_lookup_idx + n_tab * N, 0};
    return scratch_section(ctx, s, [&]() -> int {
        if (int rc = dev_keyswitch(ctx, gv, ctx->d_ms, ctx->p.log_n_poly + 1, s)) return rc;
        return dev_blind_rotate(ctx, nullptr, gv, ctx->d_ms, s, &start);
    });
} FBS_API_CATCH(ctx)

// ---- encrypted tables (include/fbs_exec.h): the wide-box map, the rotation that returns the rotated sample, the sum of samples ------
int fbs_table_map(uint32_t p, uint32_t N, uint32_t spread, uint32_t len, uint32_t base, uint32_t stride, uint32_t *map_out) try {
    return host_table_map(p, N, spread, len, base, stride, map_out);
} FBS_API_CATCH(nullptr)

// the dst_slot array of a rotation that leaves whole accumulators: the accumulator bit for every bootstrap of a pass, written when
// the array grows and never again
static int ensure_acc_flags(fbs_ctx *ctx, size_t count) {
    if (count <= ctx->acc_flags_capacity) return FBS_OK;
    if (int rc = grow(ctx, ctx->d_acc_flags, ctx->acc_flags_capacity, count, 4, false)) return rc;
    FBS_HIP(ctx, hipMemsetD32(ctx->d_acc_flags, (int)0x80000000u, count));
    FBS_HIP(ctx, hipDeviceSynchronize());
    return FBS_OK;
}

// what both rotations check once the lookups' checks are through: the flags and the output samples
static int check_rotate_out(const fbs_ctx *ctx, uint32_t flags, const uint64_t *d_glwe_out, size_t count) {
    if (flags & ~1u) return set_error(ctx, FBS_E_INVALID, "unknown flag: bit 0 (negate the amounts) is the only one");
    if (count && !d_glwe_out) return set_error(ctx, FBS_E_INVALID, "null argument");
    if ((uintptr_t)d_glwe_out & 15u) return set_error(ctx, FBS_E_INVALID, "rotated samples are GLWE samples: d_glwe_out must be 16-byte aligned");
    if (count > SIZE_MAX / 8 / ((size_t)(ctx->p.k + 1) * ctx->N)) return set_error(ctx, FBS_E_INVALID, "count * (k + 1) N words overflow");
    return FBS_OK;
}

// rows [f0, f0 + rows) of a rotation call once their amounts are in d_ms: negated where asked, then turned, whole accumulators out
static int rotate_rows(fbs_ctx *ctx, const BrStart &tables, size_t f0, size_t rows, uint32_t flags, uint64_t *d_glwe_out, hipStream_t s) {
    const uint32_t acc_words = (ctx->p.k + 1) * ctx->N;
    if ((flags & 1u))
        if (int rc = dev_ms_negate(ctx, ctx->d_ms, rows, s)) return rc;
    GateView gv = batch_view(nullptr, nullptr, nullptr, rows);
    gv.out_rows = d_glwe_out + f0 * acc_words;
    gv.row_words = acc_words;
    gv.dst_slot = ctx->d_acc_flags;
    BrStart start = tables;
    start.first = f0;
    start.whole = true;
    return dev_blind_rotate(ctx, nullptr, gv, ctx->d_ms, s, &start);
}

// (needs neither a secret nor a fold key)
int fbs_rotate_dev(fbs_ctx *ctx, const uint64_t *d_tables, uint32_t n_tables, const uint32_t *d_table_of, const uint64_t *d_cts_index,
                   size_t count, uint32_t flags, uint64_t *d_glwe_out, void *stream) try {
    if (int rc = io_prologue(ctx, d_cts_index, d_glwe_out, count, IO_CT_WORDS, nullptr)) return rc;
    if (int rc = check_lookup_tables(ctx, d_tables, n_tables, count)) return rc;
    if (int rc = check_rotate_out(ctx, flags, d_glwe_out, count)) return rc;
    if (count == 0) return FBS_OK;
    FBS_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = ensure_ms(ctx, count)) return rc;
    if (int rc = ensure_acc_flags(ctx, count)) return rc;
    const GateView gv = batch_view(d_cts_index, nullptr, nullptr, count);
    hipStream_t s = pick(ctx, stream);
    return scratch_section(ctx, s, [&]() -> int {
        if (int rc = dev_keyswitch(ctx, gv, ctx->d_ms, ctx->p.log_n_poly + 1, s)) return rc;
        return rotate_rows(ctx, BrStart{d_tables, n_tables, d_table_of, 0}, 0, count, flags, d_glwe_out, s);
    });
} FBS_API_CATCH(ctx)

// fbs_lookup_compact_dev's passes and unpack, the rotated sample out
int fbs_rotate_compact_dev(fbs_ctx *ctx, const uint64_t *d_tables, uint32_t n_tables, const uint32_t *d_table_of, const uint64_t *d_words,
                           size_t count, uint32_t bits, uint32_t flags, uint64_t *d_glwe_out, void *stream) try {
    if (int rc = io_prologue(ctx, d_words, d_glwe_out, count, IO_CT_WORDS, nullptr)) return rc;
    if (int rc = check_bits(ctx, bits)) return rc;
    if (int rc = check_compact_words(ctx, count, bits)) return rc;
    if (int rc = check_lookup_tables(ctx, d_tables, n_tables, count)) return rc;
    if (int rc = check_rotate_out(ctx, flags, d_glwe_out, count)) return rc;
    if (count == 0) return FBS_OK;
    FBS_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = ensure_acc_flags(ctx, ms_pass_size(ctx, count))) return rc;
    const size_t W = compact_words(ctx->p.n, bits);
    hipStream_t s = pick(ctx, stream);
    return ms_passes(ctx, count, s, [&](size_t f0, size_t rows) {
        if (int rc = dev_compact_unpack(ctx, d_words + f0 * W, rows, bits, ctx->d_ms, s)) return rc;
        return rotate_rows(ctx, BrStart{d_tables, n_tables, d_table_of, 0}, f0, rows, flags, d_glwe_out, s);
    });
} FBS_API_CATCH(ctx)

// dst_of is host memory: checked here, then uploaded (which blocks, as the index arrays of fbs_state_lookup do)
int fbs_glwe_add_dev(fbs_ctx *ctx, uint64_t *d_dst, size_t n_dst, const uint32_t *dst_of, const uint64_t *d_src, size_t count, void *stream) try {
    if (!ctx || (count && (!d_dst || !dst_of || !d_src))) return FBS_E_INVALID;
    if (((uintptr_t)d_dst | (uintptr_t)d_src) & 15u) return set_error(ctx, FBS_E_INVALID, "GLWE samples: d_dst and d_src must be 16-byte aligned");
    if (count > n_dst) return set_error(ctx, FBS_E_INVALID, "more sources than targets: a target would be written twice");
    if (n_dst > 0x7FFFFFFFull) return set_error(ctx, FBS_E_INVALID, "batch too large");
    if (count == 0) return FBS_OK;
    {   // the kernel reads a source word and writes a target word in no order between samples: the two arrays are disjoint
        const size_t acc_bytes = (size_t)(ctx->p.k + 1) * ctx->N * 8;
        const uintptr_t d0 = (uintptr_t)d_dst, d1 = d0 + n_dst * acc_bytes, s0 = (uintptr_t)d_src, s1 = s0 + count * acc_bytes;
        if (d0 < s1 && s0 < d1) return set_error(ctx, FBS_E_INVALID, "d_dst and d_src overlap");
    }
    for (size_t f = 0; f < count; f++)
        if (dst_of[f] >= n_dst)
            return set_error(ctx, FBS_E_INVALID, "target " + std::to_string(dst_of[f]) + " of source " + std::to_string(f) + " is past the " + std::to_string(n_dst) + " samples");
    std::vector<uint32_t> sorted(dst_of, dst_of + count);
    std::sort(sorted.begin(), sorted.end());
    const auto twice = std::adjacent_find(sorted.begin(), sorted.end());
    if (twice != sorted.end()) return set_error(ctx, FBS_E_INVALID, "target " + std::to_string(*twice) + " is written twice in one call");
    FBS_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = grow(ctx, ctx->d_add_idx, ctx->add_idx_capacity, count, 4, false)) return rc;
    if (ctx->scratch_used) FBS_HIP(ctx, hipStreamSynchronize(ctx->scratch_stream));   // (an earlier call may still read the targets)
    FBS_HIP(ctx, hipMemcpy(ctx->d_add_idx, dst_of, count * 4, hipMemcpyHostToDevice));
    hipStream_t s = pick(ctx, stream);
    return scratch_section(ctx, s, [&]() -> int { return dev_glwe_add(ctx, d_dst, d_src, ctx->d_add_idx, count, s); });
} FBS_API_CATCH(ctx)

// ---- resident tables: folded samples that persist, read by rotation and written by rotation ---------------------------------------
static bool table_of_ctx(const fbs_ctx *ctx, const fbs_table *t) {   // (by address, as state_of)
    return t && std::find(ctx->tables.begin(), ctx->tables.end(), t) != ctx->tables.end();
}

// the maps of n_tab tables from one wide-box layout `box` (entry numbers: host_table_map at base 0, stride 1): table t's entry x
// is source src(t, x)
static void table_maps(uint32_t *maps, const std::vector<uint32_t> &box, size_t n_tab, const std::function<uint32_t(size_t, uint32_t)> &src) {
    const size_t N = box.size();
    for (size_t t = 0; t < n_tab; t++)
        for (size_t j = 0; j < N; j++)
            maps[t * N + j] = box[j] == FOLD_MAP_NONE ? FOLD_MAP_NONE : src(t, box[j] & ~FOLD_MAP_NEG) | (box[j] & FOLD_MAP_NEG);
}

// the index arrays of a table call, uploaded once (which blocks: an earlier call may still read them)
static int upload_table_idx(fbs_ctx *ctx, const std::vector<uint32_t> &idx) {
    if (int rc = grow(ctx, ctx->d_lookup_idx, ctx->lookup_idx_capacity, idx.size(), 4, false)) return rc;
    if (ctx->scratch_used) FBS_HIP(ctx, hipStreamSynchronize(ctx->scratch_stream));
    FBS_HIP(ctx, hipMemcpy(ctx->d_lookup_idx, idx.data(), idx.size() * 4, hipMemcpyHostToDevice));
    return FBS_OK;
}

int fbs_table_create(fbs_ctx *ctx, const fbs_state *state, const uint32_t *rows, uint32_t n_planes, uint32_t len, uint32_t spread,
                     fbs_table **out) try {
    if (!ctx || !out) return FBS_E_INVALID;
    *out = nullptr;
    if (!state_of(ctx, state)) return set_error(ctx, FBS_E_INVALID, "not a live state of this context");
    if (!rows || n_planes == 0) return set_error(ctx, FBS_E_INVALID, "a table set has at least one plane");
    const uint32_t N = ctx->N, p = ctx->p.p_msg, k1 = ctx->p.k + 1;
    if (spread < 1) return set_error(ctx, FBS_E_INVALID, "an entry takes at least one box");
    if (len == 0) return set_error(ctx, FBS_E_INVALID, "a table has at least one entry");
    if (len > p / spread) return set_error(ctx, FBS_E_INVALID, "a table has at most floor(p / spread) entries");
    const size_t T = state->T, n_tab = (size_t)n_planes * T, n_src = state->rows * T;
    for (size_t i = 0; i < (size_t)n_planes * len; i++)
        if (rows[i] >= state->rows) return set_error(ctx, FBS_E_INVALID, "rows past the end of the state");
    if (n_src >= FOLD_MAP_NEG || n_tab > 0x7FFFFFFFull / N) return set_error(ctx, FBS_E_INVALID, "batch too large");
    if (int rc = gadget_prologue(ctx, GK_FOLD, n_tab * N, 0)) return rc;
    FBS_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<uint32_t> box(N), idx(n_tab * N);
    if (int rc = host_table_map(p, N, spread, len, 0, 1, box.data())) return rc;
    table_maps(idx.data(), box, n_tab, [&](size_t t, uint32_t x) { return (uint32_t)((size_t)rows[t / T * len + x] * T + t % T); });
    std::unique_ptr<fbs_table> tab(new fbs_table);
    ctx->tables.reserve(ctx->tables.size() + 1);
    const size_t bytes = n_tab * k1 * N * 8;
    const hipError_t e = hipMalloc(&tab->d, bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return set_error(ctx, FBS_E_DEVICE, "tables of " + std::to_string(bytes) + " bytes: " + hipGetErrorString(e));
    }
    int rc = upload_table_idx(ctx, idx);
    if (rc == FBS_OK) rc = gadget_passes(ctx, GK_FOLD, state->d, n_tab * N, 0, tab->d, nullptr, ctx->stream, ctx->d_lookup_idx, n_src);
    if (rc == FBS_OK) {   // the unit boxes of the writes to come, made and uploaded once: unit t holds ciphertext t of a write's scratch
        if ((rc = host_table_map(p, N, spread, 1, 0, 1, box.data())) == FBS_OK) {
            table_maps(idx.data(), box, n_tab, [](size_t t, uint32_t) { return (uint32_t)t; });
            if (hipMalloc(&tab->d_unit_maps, idx.size() * 4) != hipSuccess ||
                hipMemcpy(tab->d_unit_maps, idx.data(), idx.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
                (void)hipGetLastError();
                rc = set_error(ctx, FBS_E_DEVICE, "the unit-box maps of " + std::to_string(idx.size() * 4) + " bytes could not be placed");
            }
        }
    }
    if (rc != FBS_OK) {
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipFree(tab->d);
        if (tab->d_unit_maps) (void)hipFree(tab->d_unit_maps);
        return rc;
    }
    tab->ctx = ctx, tab->n_tab = n_tab, tab->T = T, tab->n_planes = n_planes, tab->len = len, tab->spread = spread;
    ctx->tables.push_back(tab.get());
    *out = tab.release();
    return FBS_OK;
} FBS_API_CATCH(ctx)

void fbs_table_free(fbs_table *table) try {
    if (!table) return;
    fbs_ctx *ctx = table->ctx;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);   // queued reads and writes may still use it
    if (ctx->scratch_used) (void)hipStreamSynchronize(ctx->scratch_stream);
    ctx->tables.erase(std::remove(ctx->tables.begin(), ctx->tables.end(), table), ctx->tables.end());
    (void)hipFree(table->d);
    (void)hipFree(table->d_unit_maps);
    delete table;
} catch (...) {
}

int fbs_table_stat(const fbs_table *table, const char *name, int64_t *value) try {
    if (!table || !name || !value) return FBS_E_INVALID;
    const std::string k(name);
    if (k == "tables") *value = (int64_t)table->n_tab;
    else if (k == "planes") *value = table->n_planes;
    else if (k == "samples") *value = (int64_t)table->T;
    else if (k == "len") *value = table->len;
    else if (k == "spread") *value = table->spread;
    else if (k == "writes") *value = table->writes;
    else if (k == "words") *value = (int64_t)(table->n_tab * (table->ctx->p.k + 1) * table->ctx->N);
    else return set_error(table->ctx, FBS_E_INVALID, "unknown statistic '" + k + "'");
    return FBS_OK;
} FBS_API_CATCH(table ? table->ctx : nullptr)

int fbs_table_words(fbs_ctx *ctx, const fbs_table *table, uint64_t *out) try {
    if (!ctx || !out) return FBS_E_INVALID;
    if (!table_of_ctx(ctx, table)) return set_error(ctx, FBS_E_INVALID, "not a live table of this context");
    FBS_HIP(ctx, hipSetDevice(ctx->device));
    FBS_HIP(ctx, hipMemcpyAsync(out, table->d, table->n_tab * (ctx->p.k + 1) * ctx->N * 8, hipMemcpyDeviceToHost, ctx->stream));
    return sync_stream(ctx, ctx->stream);
} FBS_API_CATCH(ctx)

// what a read and a write check of the index: its state and row, and that its samples are the table's (or, shared, any -- a write: one)
static int check_table_index(const fbs_ctx *ctx, const fbs_table *table, const fbs_state *index_state, size_t index_row, bool writing) {
    if (!table_of_ctx(ctx, table)) return set_error(ctx, FBS_E_INVALID, "not a live table of this context");
    if (!state_of(ctx, index_state)) return set_error(ctx, FBS_E_INVALID, "not a live state of this context");
    if (index_row >= index_state->rows) return set_error(ctx, FBS_E_INVALID, "rows past the end of the state");
    if (table->T != 1 && index_state->T != table->T) return set_error(ctx, FBS_E_INVALID, "the index state has not the tables' samples");
    if (writing && table->T == 1 && index_state->T != 1)
        return set_error(ctx, FBS_E_INVALID, "a shared table is written by an index state of one sample: several samples writing one table in one call have no order");
    if ((size_t)table->n_planes * index_state->T > 0x7FFFFFFFull) return set_error(ctx, FBS_E_INVALID, "batch too large");
    return FBS_OK;
}

// the view in which the planes of an index share its one key switch: bootstrap f = m T + s, source_of all zero
static GateView table_view(const fbs_ctx *ctx, const fbs_table *table, const fbs_state *index_state, size_t index_row, const uint32_t *d_zeros) {
    const size_t T = index_state->T;
    GateView gv{};
    gv.in_base = index_state->d + index_row * T * (ctx->D + 1);
    gv.source_of = d_zeros;
    gv.T = T, gv.s_count = T, gv.count = (size_t)table->n_planes * T, gv.ks_count = T, gv.n_gates = table->n_planes;
    return gv;
}

// fbs_state_lookup's rotation without its fold
int fbs_table_read(fbs_ctx *ctx, const fbs_table *table, const fbs_state *index_state, size_t index_row, fbs_state *out_state,
                   size_t out_row0) try {
    if (!ctx) return FBS_E_INVALID;
    if (int rc = check_table_index(ctx, table, index_state, index_row, false)) return rc;
    if (!state_of(ctx, out_state)) return set_error(ctx, FBS_E_INVALID, "not a live state of this context");
    if (out_state == index_state) return set_error(ctx, FBS_E_INVALID, "the output state must be another state");
    const size_t T = index_state->T, count = (size_t)table->n_planes * T;
    if (out_state->T != T || out_row0 > out_state->rows || table->n_planes > out_state->rows - out_row0)
        return set_error(ctx, FBS_E_INVALID, "the output state holds n_planes rows of the index state's samples from out_row0 on");
    if (!ctx->have_keys) return set_error(ctx, FBS_E_STATE, "fbs_keygen has not run");
    FBS_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<uint32_t> idx(count + table->n_planes, 0u);   // which table a bootstrap reads, then the planes' shared source
    for (size_t f = 0; f < count; f++) idx[f] = (uint32_t)(table->T == 1 ? f / T : f);
    if (int rc = ensure_ms(ctx, T)) return rc;
    if (int rc = upload_table_idx(ctx, idx)) return rc;
    GateView gv = table_view(ctx, table, index_state, index_row, ctx->d_lookup_idx + count);
    gv.out_base = out_state->d + out_row0 * T * (ctx->D + 1);
    const BrStart start{table->d, (uint32_t)table->n_tab, ctx->d_lookup_idx, 0};
    hipStream_t s = ctx->stream;
    return scratch_section(ctx, s, [&]() -> int {
        if (int rc = dev_keyswitch(ctx, gv, ctx->d_ms, ctx->p.log_n_poly + 1, s)) return rc;
        return dev_blind_rotate(ctx, nullptr, gv, ctx->d_ms, s, &start);
    });
} FBS_API_CATCH(ctx)

// ADD: the values folded into unit boxes, turned by the index's negated amounts, added.  SET: first the old entries read by the same
// amounts, refreshed, and taken off the values; then the add steps on the differences.  Bootstrap f = m T + s writes table f.
int fbs_table_write(fbs_ctx *ctx, fbs_table *table, const fbs_state *index_state, size_t index_row, const fbs_state *value_state,
                    const uint32_t *value_rows, uint32_t mode, const fbs_tvset *identity) try {
    if (!ctx) return FBS_E_INVALID;
    if (mode > 1) return set_error(ctx, FBS_E_INVALID, "mode is 0 (add) or 1 (set)");
    if (int rc = check_table_index(ctx, table, index_state, index_row, true)) return rc;
    if (!state_of(ctx, value_state)) return set_error(ctx, FBS_E_INVALID, "not a live state of this context");
    if (!value_rows) return set_error(ctx, FBS_E_INVALID, "null argument");
    const size_t T = index_state->T, count = table->n_tab, n_planes = table->n_planes;
    const uint32_t N = ctx->N, acc_words = (ctx->p.k + 1) * N;
    const size_t ctw = ctx->D + 1;
    if (value_state->T != T) return set_error(ctx, FBS_E_INVALID, "the value state has not the index state's samples");
    for (size_t m = 0; m < n_planes; m++)
        if (value_rows[m] >= value_state->rows) return set_error(ctx, FBS_E_INVALID, "rows past the end of the state");
    const size_t n_values = value_state->rows * T;
    if (n_values >= FOLD_MAP_NEG) return set_error(ctx, FBS_E_INVALID, "batch too large");
    if (int rc = gadget_prologue(ctx, GK_FOLD, count * N, 0)) return rc;
    FBS_HIP(ctx, hipSetDevice(ctx->device));
    fbs_tvset *tv = nullptr;
    if (mode == 1) {
        if (identity && identity->ctx != ctx) return set_error(ctx, FBS_E_INVALID, "test-vector set belongs to another context");
        if (!identity)
            if (int rc = identity_tv(ctx, &tv)) return rc;
    }
    const fbs_tvset *refresh = identity ? identity : tv;
    // the index arrays of the call, a few words a table: the value of table f [count], 0 .. count - 1 [count], zeros [n_planes].  The
    // unit-box maps, N words a table, are the table object's own (made once by fbs_table_create): unit f folds ciphertext f of the
    // scratch, where an add gathers its values and a set leaves its differences, in the tables' order
    std::vector<uint32_t> idx(2 * count + n_planes, 0u);
    uint32_t *value_of = idx.data(), *ident = value_of + count;
    for (size_t f = 0; f < count; f++) value_of[f] = (uint32_t)((size_t)value_rows[f / T] * T + f % T), ident[f] = (uint32_t)f;
    const size_t units = 0, turned = count * acc_words, olds = 2 * count * acc_words;   // offsets into the scratch, in words
    if (int rc = grow(ctx, ctx->d_table_scratch, ctx->table_scratch_capacity, olds + count * ctw, 8, true)) return rc;
    if (int rc = ensure_ms(ctx, mode == 1 ? std::max(T, count) : T)) return rc;
    if (int rc = ensure_acc_flags(ctx, n_planes)) return rc;
    if (int rc = upload_table_idx(ctx, idx)) return rc;
    const uint32_t *d_value_of = ctx->d_lookup_idx, *d_ident = d_value_of + count, *d_zeros = d_ident + count;
    uint64_t *d_units = ctx->d_table_scratch + units, *d_turned = ctx->d_table_scratch + turned, *d_old = ctx->d_table_scratch + olds;
    const GateView gv = table_view(ctx, table, index_state, index_row, d_zeros);
    const uint32_t log2_mod = ctx->p.log_n_poly + 1;
    hipStream_t s = ctx->stream;
    {
        int rc = scratch_section(ctx, s, [&]() -> int {
            if (mode == 0) return dev_ct_sub(ctx, value_state->d, d_value_of, nullptr, d_old, count, s);   // (nothing taken off: a gather)
            if (int rc = dev_keyswitch(ctx, gv, ctx->d_ms, log2_mod, s)) return rc;
            GateView read = gv;
            read.out_rows = d_old;   // (rows of D + 1 words: table f's old entry is ciphertext f)
            const BrStart start{table->d, (uint32_t)count, nullptr, 0};
            if (int rc = dev_blind_rotate(ctx, nullptr, read, ctx->d_ms, s, &start)) return rc;
            // refreshed: a written box would otherwise carry the table's noise twice over after every set
            if (int rc = dev_keyswitch(ctx, batch_view(d_old, nullptr, nullptr, count), ctx->d_ms, log2_mod, s)) return rc;
            if (int rc = dev_blind_rotate(ctx, refresh, batch_view(nullptr, d_old, nullptr, count), ctx->d_ms, s)) return rc;
            return dev_ct_sub(ctx, value_state->d, d_value_of, d_old, d_old, count, s);
        });
        if (rc != FBS_OK) return rc;
    }
    if (int rc = gadget_passes(ctx, GK_FOLD, d_old, count * N, 0, d_units, nullptr, s, table->d_unit_maps, count)) return rc;
    int rc = scratch_section(ctx, s, [&]() -> int {
        if (int rc = dev_keyswitch(ctx, gv, ctx->d_ms, log2_mod, s)) return rc;   // (a set's refresh has used the amounts' rows)
        if (int rc = dev_ms_negate(ctx, ctx->d_ms, T, s)) return rc;
        GateView turn = gv;
        turn.out_rows = d_turned;
        turn.row_words = acc_words;
        turn.dst_slot = ctx->d_acc_flags;
        BrStart start{d_units, (uint32_t)count, nullptr, 0};
        start.whole = true;
        if (int rc = dev_blind_rotate(ctx, nullptr, turn, ctx->d_ms, s, &start)) return rc;
        return dev_glwe_add(ctx, table->d, d_turned, d_ident, count, s);
    });
    if (rc == FBS_OK) table->writes++;
    return rc;
} FBS_API_CATCH(ctx)

int fbs_state_fold(fbs_ctx *ctx, const fbs_state *st, size_t row0, size_t rows, uint64_t *out) try {
    if (!ctx) return FBS_E_INVALID;
    if (int rc = check_state_rows(ctx, st, row0, rows, out)) return rc;
    const StateSpan span = state_span(ctx, st, row0, rows);
    if (int rc = gadget_prologue(ctx, GK_FOLD, span.count, 0)) return rc;
    if (rows == 0) return FBS_OK;
    return gadget_passes(ctx, GK_FOLD, span.d, span.count, 0, nullptr, out, ctx->stream);
} FBS_API_CATCH(ctx)

int fbs_state_fold_dev(fbs_ctx *ctx, const fbs_state *st, size_t row0, size_t rows, uint64_t *d_glwe) try {
    if (!ctx) return FBS_E_INVALID;
    if (int rc = check_state_rows(ctx, st, row0, rows, d_glwe)) return rc;
    const StateSpan span = state_span(ctx, st, row0, rows);
    if (int rc = gadget_prologue(ctx, GK_FOLD, span.count, 0)) return rc;
    if (int rc = check_fold_target(ctx, d_glwe)) return rc;
    if (rows == 0) return FBS_OK;
    return gadget_passes(ctx, GK_FOLD, span.d, span.count, 0, d_glwe, nullptr, ctx->stream);
} FBS_API_CATCH(ctx)

// the device-source twin of fbs_state_put_public: no staging, no check of the words (device memory), queued on the context's stream
int fbs_state_unfold_dev(fbs_ctx *ctx, fbs_state *st, size_t row0, size_t rows, const uint64_t *d_glwe) try {
    if (!ctx) return FBS_E_INVALID;
    if (int rc = check_state_rows(ctx, st, row0, rows, d_glwe)) return rc;
    if (rows == 0) return FBS_OK;
    FBS_HIP(ctx, hipSetDevice(ctx->device));
    const StateSpan span = state_span(ctx, st, row0, rows);
    return dev_expand_public(ctx, d_glwe, span.count, span.d, ctx->stream);
} FBS_API_CATCH(ctx)

// test hook of the front kernel alone: d_cts [count][D + 1] -> d_fields [D][cols] uint32 rounded to tg bits, then cols 64-bit body
// words; cols a multiple of N with count <= cols.  Needs no key.
int fbs_debug_fold_front_dev(fbs_ctx *ctx, const uint64_t *d_cts, size_t count, uint32_t cols, uint32_t tg, uint32_t *d_fields, void *stream) try {
    if (!ctx || !d_fields || (count && !d_cts)) return FBS_E_INVALID;
    if (tg < 1 || tg > 31) return set_error(ctx, FBS_E_INVALID, "the fields are rounded to 1 .. 31 bits");
    if (cols == 0 || cols % ctx->N || count > cols || cols > (1u << 20))
        return set_error(ctx, FBS_E_INVALID, "cols is a multiple of N, at most 2^20, that holds the ciphertexts");
    if ((uintptr_t)d_fields & 7u) return set_error(ctx, FBS_E_INVALID, "d_fields must be 8-byte aligned");
    FBS_HIP(ctx, hipSetDevice(ctx->device));
    return dev_fold_front(ctx, d_cts, count, cols, tg, d_fields, pick(ctx, stream));
} FBS_API_CATCH(ctx)

// ---------------------------------------------------------------------------------------------
int fbs_profile_enable(fbs_ctx *ctx, int on) try {
    if (!ctx) return FBS_E_INVALID;
    ctx->prof.on = on != 0;
    return FBS_OK;
} FBS_API_CATCH(ctx)

static int profile_collect(fbs_ctx *ctx) {
    FBS_HIP(ctx, hipSetDevice(ctx->device));
    for (int k = 0; k < 3; k++) {
        for (auto &pr : ctx->prof.pending[k]) {
            FBS_HIP(ctx, hipEventSynchronize(pr.end));
            float t = 0;
            FBS_HIP(ctx, hipEventElapsedTime(&t, pr.begin, pr.end));
            ctx->prof.ms[k] += t;
            ctx->prof.launches[k]++;
            Profile::PerKernel &pk = ctx->prof.by_kernel[k][pr.kernel];
            pk.ms += t;
            pk.launches++;
            ctx->prof.pool.push_back({pr.begin, pr.end});
        }
        ctx->prof.pending[k].clear();
    }
    return FBS_OK;
}

int fbs_profile_read(fbs_ctx *ctx, double ms[3], uint64_t launches[3], int reset) try {
    if (!ctx) return FBS_E_INVALID;
    if (int rc = profile_collect(ctx)) return rc;
    for (int k = 0; k < 3; k++) {
        if (ms) ms[k] = ctx->prof.ms[k];
        if (launches) launches[k] = ctx->prof.launches[k];
        if (reset) {
            ctx->prof.ms[k] = 0;
            ctx->prof.launches[k] = 0;
            ctx->prof.by_kernel[k].clear();
        }
    }
    return FBS_OK;
} FBS_API_CATCH(ctx)

int fbs_profile_kernels(fbs_ctx *ctx, char *buf, size_t cap, size_t *needed) try {
    if (!ctx) return FBS_E_INVALID;
    if (int rc = profile_collect(ctx)) return rc;
    std::string text;
    for (int k = 0; k < 3; k++)
        for (const auto &kv : ctx->prof.by_kernel[k]) {
            char line[64];
            snprintf(line, sizeof line, "\t%llu\t%.6f\n", (unsigned long long)kv.second.launches, kv.second.ms);
            text += std::to_string(k) + "\t" + kv.first + line;
        }
    if (needed) *needed = text.size() + 1;
    if (!buf || cap < text.size() + 1) return buf ? set_error(ctx, FBS_E_INVALID, "buffer too small") : FBS_OK;
    std::memcpy(buf, text.c_str(), text.size() + 1);
    return FBS_OK;
} FBS_API_CATCH(ctx)

const char *fbs_profile_kernel(const fbs_ctx *ctx, int which) try {
    if (!ctx || which < 0 || which > 2) return "";
    return ctx->prof.kernel[which].c_str();
} catch (...) { return ""; }

const char *fbs_kernel_catalog(void) try {
    static const std::string text = [] {
        std::vector<std::string> names;
        kernel_catalog(&names);
        std::string t;
        for (const std::string &n : names) t += n + "\n";
        return t;
    }();
    return text.c_str();
} catch (...) { return ""; }

int fbs_sync(fbs_ctx *ctx, void *stream) try {
    if (!ctx) return FBS_E_INVALID;
    FBS_HIP(ctx, hipSetDevice(ctx->device));
    FBS_HIP(ctx, hipStreamSynchronize(pick(ctx, stream)));
    return FBS_OK;
} FBS_API_CATCH(ctx)

int fbs_debug_polymul(fbs_ctx *ctx, const uint64_t *a, const uint64_t *b, uint64_t *c) try {
    int rc = check_ready(ctx, nullptr);
    if (rc != FBS_OK) return rc;
    const size_t bytes = (size_t)ctx->N * 8;
    uint64_t *d = nullptr;
    FBS_HIP(ctx, hipMalloc(&d, 3 * bytes));
    hipError_t e = hipMemcpy(d, a, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + ctx->N, b, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        rc = dev_polymul(ctx, d, d + ctx->N, d + 2 * (size_t)ctx->N, ctx->stream);
        if (rc == FBS_OK) e = hipStreamSynchronize(ctx->stream);
    }
    if (e == hipSuccess && rc == FBS_OK) e = hipMemcpy(c, d + 2 * (size_t)ctx->N, bytes, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (rc != FBS_OK) return rc;
    if (e != hipSuccess) return set_error(ctx, FBS_E_DEVICE, std::string("polymul: ") + hipGetErrorString(e));
    return FBS_OK;
} FBS_API_CATCH(ctx)

int fbs_debug_field(fbs_ctx *ctx, int op, const int64_t *x, const int64_t *w, size_t count, int64_t *out) try {
    int rc = check_ready(ctx, nullptr);
    if (rc != FBS_OK) return rc;
    return dev_debug_field(ctx, op, x, w, count, out);
} FBS_API_CATCH(ctx)

const char *fbs_debug_transform_list(void) try {
    return debug_transform_list();
} catch (...) { return ""; }

int fbs_debug_transform(fbs_ctx *ctx, const char *variant, const int64_t *in, int64_t *out, size_t polys) try {
    int rc = check_ready(ctx, nullptr);
    if (rc != FBS_OK) return rc;
    return dev_debug_transform(ctx, variant, in, out, polys);
} FBS_API_CATCH(ctx)

// test hooks of the rounded Gaussian (fbs_sampler.hpp) on raw windows of words, whatever the context's own sampler: on the host
// (no context needed: the sampler has no state, ctx only takes the error text) and on the device with one thread per window
int fbs_debug_gauss(const fbs_ctx *ctx, const uint64_t *words, size_t count, uint64_t sigma, int64_t *out) try {
    if (const char *why = debug_gauss_refused(words, count, sigma, out)) return set_error(ctx, FBS_E_INVALID, why);
    host_debug_gauss(words, count, sigma, out);
    return FBS_OK;
} FBS_API_CATCH(ctx)

int fbs_debug_gauss_dev(fbs_ctx *ctx, const uint64_t *d_words, size_t count, uint64_t sigma, int64_t *d_out, void *stream) try {
    if (!ctx) return FBS_E_INVALID;
    if (const char *why = debug_gauss_refused(d_words, count, sigma, d_out)) return set_error(ctx, FBS_E_INVALID, why);
    if (count == 0) return FBS_OK;
    FBS_HIP(ctx, hipSetDevice(ctx->device));
    return dev_debug_gauss(ctx, d_words, count, sigma, d_out, pick(ctx, stream));
} FBS_API_CATCH(ctx)

// test hook of the packing kernels: fbs_pack_dev without its key switch, on fields [count][n + 1] at 31 bits that a test supplies --
// mask fields no key switch under seeded keys could be made to give.  One pass of fbs_pack_dev: its scratch growth, then dev_pack
// on the caller's pointer in place of the modulus-switch scratch.
int fbs_debug_pack_fields_dev(fbs_ctx *ctx, const uint32_t *d_fields, size_t count, uint32_t bits, uint64_t *d_words, void *stream) try {
    if (int rc = io_prologue(ctx, d_fields, d_words, count, 0, nullptr)) return rc;
    if (int rc = gadget_prologue(ctx, GK_PACK, count, bits)) return rc;
    if (count == 0) return FBS_OK;
    if (count > std::max(ctx->ms_capacity, COMPACT_PASS) / ctx->N * ctx->N)
        return set_error(ctx, FBS_E_INVALID, "more fields than one pass of fbs_pack_dev holds");
    FBS_HIP(ctx, hipSetDevice(ctx->device));
    size_t pass = 0;
    if (int rc = pack_reserve(ctx, count, &pass)) return rc;
    hipStream_t s = pick(ctx, stream);
    return scratch_section(ctx, s, [&] { return dev_pack(ctx, d_fields, count, bits, d_words, s); });
} FBS_API_CATCH(ctx)

}  // extern "C"

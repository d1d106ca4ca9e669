// Host side of libfbsexec.so: key generation, encryption/decryption and test-vector construction.
// None of this is on the timed path; it exists so that the drop-in `LutExecEnv.eval`
// (reference fbs_mapper/fbs_exec_env.py:208-229) can take cleartext bits in and hand cleartext
// values back, as the reference's harness (fbs_mapper/map_circuit.py:137-180) expects.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <functional>
#include <cstring>
#include <thread>

#include "fbs_internal.hpp"
#include "fbs_chacha.hpp"
#include "fbs_sampler.hpp"
#include "fbs_compact.hpp"
#include "fbs_pack.hpp"

namespace fbs {

// ---------------------------------------------------------------------------------------------
// ChaCha20 (fbs_chacha.hpp, the same code the device encryption runs): original 64-bit-counter layout, key = seed || fixed
// tail, stream id in the nonce words.
// ---------------------------------------------------------------------------------------------
RandKey rand_key_from_seed64(uint64_t seed) {
    // key words 2..7 spell "fbs-exec-amd-gfx950-key1"
    static const uint32_t tail[6] = {0x2d736266u, 0x63657865u, 0x646d612du, 0x7866672du, 0x2d303539u, 0x3179656bu};
    RandKey k;
    k.w[0] = (uint32_t)seed;
    k.w[1] = (uint32_t)(seed >> 32);
    for (int i = 0; i < 6; i++) k.w[2 + i] = tail[i];
    return k;
}

// 32 bytes of caller entropy -> the context's key: one ChaCha block under the caller's bytes, on a stream named by the
// parameter set, so that contexts with different parameters under one seed share no key material (their secret keys would
// otherwise be prefixes of each other).
RandKey rand_key_derive(const uint8_t seed[32], const fbs_params &p) {
    RandKey master;
    std::memcpy(master.w, seed, 32);
    uint64_t h = 0xcbf29ce484222325ull;   // FNV-1a over the fields that define the key material
    const uint64_t fields[] = {p.n, p.log_n_poly, p.k, p.l_bsk, p.beta_bsk, p.t_ksk, p.gamma_ksk, p.p_msg, p.sigma_lwe, p.sigma_glwe,
                               p.bsk_group == 2 ? 2u : 1u};
    auto mix = [&h](uint64_t f) {
        for (int b = 0; b < 8; b++) {
            h ^= (f >> (8 * b)) & 0xff;
            h *= 0x100000001b3ull;
        }
    };
    for (uint64_t f : fields) mix(f);
    if (p.sampler) mix(p.sampler);   // (only then: the derivations of sampler 0 stay what they were)
    uint64_t blk[8];
    chacha_block(master.w, (0xFFull << 56) | (h & 0x00FFFFFFFFFFFFFFull), 0, blk);
    RandKey k;
    std::memcpy(k.w, blk, 32);
    return k;
}

void rand_words(const RandKey &seed, uint64_t stream, uint64_t idx0, uint64_t *dst, size_t count) {
    uint64_t blk[8];
    uint64_t have = ~0ull;
    for (size_t i = 0; i < count; i++) {
        uint64_t idx = idx0 + i;
        if ((idx >> 3) != have) {
            have = idx >> 3;
            chacha_block(seed.w, stream, have, blk);
        }
        dst[i] = blk[idx & 7];
    }
}

// sample idx of a stream: the sampler (fbs_sampler.hpp: 0 irwin_hall_sample, 1 gauss_sample) applied to its words 6 idx .. 6 idx + 5;
// no draw when sigma is 0
int64_t noise_sample(const RandKey &seed, uint64_t stream, uint64_t idx, uint64_t sigma, uint32_t sampler) {
    if (!sigma) return 0;
    uint64_t w[6];
    rand_words(seed, stream, idx * 6, w, 6);
    return sample_window(sampler, w, sigma);
}

// ---------------------------------------------------------------------------------------------
// The two samples everything here encrypts with (the device's frame of the first is fbs_rows.hpp, of the second k_glwe_key_rows).
// An LWE row: mask_words, then lwe_body + the caller's message.  A GLWE zero sample: glwe_zero_sample, then the caller's message.
// ---------------------------------------------------------------------------------------------
void mask_words(const RandKey &key, uint64_t stream, uint64_t idx0, uint64_t *dst, size_t len) {
    rand_words(key, stream, idx0, dst, len);
    for (size_t i = 0; i < len; i++) dst[i] = fq_fold(dst[i]);
}

uint64_t lwe_body(const RandKey &noise_key, uint64_t noise_stream, uint64_t sigma, uint32_t sampler, const uint64_t *mask,
                  const uint64_t *sk, size_t len) {
    uint64_t b = fq_from_i64(noise_sample(noise_key, noise_stream, 0, sigma, sampler));
    for (size_t i = 0; i < len; i++)
        if (sk[i]) b = fq_add(b, mask[i]);
    return b;
}

void add_times_key(uint64_t *acc, const uint64_t *a, const std::vector<uint32_t> &support, uint32_t N) {
    for (uint32_t sh : support) {
        for (uint32_t j = 0; j < N - sh; j++) acc[j + sh] = fq_add(acc[j + sh], a[j]);
        for (uint32_t j = N - sh; j < N; j++) acc[j + sh - N] = fq_sub(acc[j + sh - N], a[j]);
    }
}

void glwe_zero_sample(const RandKey &mask_key, uint64_t mask_stream, const RandKey &noise_key, uint64_t noise_stream, uint64_t sigma,
                      uint32_t sampler, const std::vector<std::vector<uint32_t>> &support, uint32_t N, uint64_t *masks, uint64_t *body) {
    for (uint32_t j = 0; j < N; j++) body[j] = fq_from_i64(noise_sample(noise_key, noise_stream, j, sigma, sampler));
    for (size_t c = 0; c < support.size(); c++) {
        mask_words(mask_key, mask_stream, c * N, masks + c * N, N);
        add_times_key(body, masks + c * N, support[c], N);
    }
}

const char *debug_gauss_refused(const void *words, size_t count, uint64_t sigma, const void *out) {
    if (count && (!words || !out)) return "debug_gauss: null array";
    if (count > ((size_t)1 << 26)) return "debug_gauss: too many windows";
    if (sigma > FQ) return "debug_gauss: sigma above q";
    return nullptr;
}

void host_debug_gauss(const uint64_t *words, size_t count, uint64_t sigma, int64_t *out) {
    for (size_t i = 0; i < count; i++) out[i] = gauss_sample(words + 6 * i, sigma);
}

// Worker threads of parallel_for: OMP_NUM_THREADS when it is set to a positive number (the usual way a machine tells a process how
// many CPUs are its own: a pool sized by a shared machine's CPU count only slows itself down), else the hardware's count.
static unsigned worker_count() {
    if (const char *env = std::getenv("OMP_NUM_THREADS")) {
        char *end = nullptr;
        const long v = std::strtol(env, &end, 10);
        if (end != env && v >= 1) return (unsigned)std::min<long>(v, 1024);
    }
    return std::max(1u, std::thread::hardware_concurrency());
}

static void parallel_for(size_t n, const std::function<void(size_t, size_t)> &body) {
    unsigned hw = worker_count();
    size_t workers = std::min<size_t>(hw, std::max<size_t>(1, n));
    if (workers <= 1) {
        body(0, n);
        return;
    }
    std::vector<std::thread> pool;
    size_t chunk = (n + workers - 1) / workers;
    for (size_t w = 0; w < workers; w++) {
        size_t a = w * chunk, b = std::min(n, a + chunk);
        if (a >= b) break;
        pool.emplace_back([=, &body] { body(a, b); });
    }
    for (auto &t : pool) t.join();
}

// ---------------------------------------------------------------------------------------------
// keys
// ---------------------------------------------------------------------------------------------
// What a context derives from its parameter set before any device is involved: range checks, sizes, Delta = 2 round(q / 4p),
// the gadget factors g_l = round(q / 2^(beta (l+1))), h_v = round(q / 2^(gamma (v+1))), and the key all randomness is expanded from.
int host_ctx_init(fbs_ctx *ctx, const fbs_params *params, uint64_t seed, const uint8_t *seed32) {
    ctx->p = *params;
    ctx->seed = seed;
    ctx->rkey = seed32 ? rand_key_derive(seed32, *params) : rand_key_from_seed64(seed);
    ctx->mask_key = mask_key_of(ctx->rkey);
    const fbs_params &p = ctx->p;
    if (p.log_n_poly < 2 || p.log_n_poly > 14 || p.k < 1 || p.k > 4 || p.p_msg < 1 || p.p_msg > 4096 || p.l_bsk > 16 ||
        p.t_ksk > 64)
        return set_error(ctx, FBS_E_INVALID, "parameter out of range");
    if (p.bsk_group > 2 || (p.bsk_group == 2 && (p.n & 1)))
        return set_error(ctx, FBS_E_INVALID, "bsk_group is 0, 1 or 2, and 2 needs an even n");
    if (p.sampler > SAMPLER_GAUSS) return set_error(ctx, FBS_E_INVALID, "sampler is 0 (Irwin-Hall) or 1 (rounded Gaussian)");
    if (p.sampler == SAMPLER_GAUSS && (p.sigma_lwe > FQ || p.sigma_glwe > FQ))
        return set_error(ctx, FBS_E_INVALID, "the rounded Gaussian takes standard deviations up to q");
    ctx->N = 1u << p.log_n_poly;
    ctx->D = p.k * ctx->N;
    ctx->rows = (p.k + 1) * p.l_bsk;
    ctx->group = p.bsk_group == 2 ? 2 : 1;
    ctx->n_ggsw = ctx->group == 2 ? (size_t)p.n / 2 * 3 : p.n;
    ctx->ksk_stride = ((p.n + 1 + 255) / 256) * 256;
    ctx->delta_half = (uint64_t)(((unsigned __int128)FQ + 2ull * p.p_msg) / (4ull * p.p_msg));
    if (const char *why = params_out_of_range(p, ctx->D)) return set_error(ctx, FBS_E_INVALID, why);   // (before the shifts below)
    auto round_div = [](uint32_t e) {
        unsigned __int128 d = (unsigned __int128)1 << e;
        return (uint64_t)(((unsigned __int128)FQ + d / 2) / d);
    };
    for (uint32_t lv = 0; lv < p.l_bsk; lv++) ctx->g[lv] = round_div(p.beta_bsk * (lv + 1));
    for (uint32_t v = 0; v < p.t_ksk; v++) ctx->h[v] = round_div(p.gamma_ksk * (v + 1));
    return FBS_OK;
}

// the secret keys of fbs_keygen and fbs_keygen_seeded alike (DOM_SK_LWE, DOM_SK_GLWE)
void draw_secrets(fbs_ctx *ctx) {
    const uint32_t n = ctx->p.n, D = ctx->D;
    ctx->sk_lwe.assign(n, 0);
    ctx->sk_glwe.assign(D, 0);
    std::vector<uint64_t> w(std::max(n, D));
    rand_words(ctx->rkey, stream_id(DOM_SK_LWE, 0), 0, w.data(), n);
    for (uint32_t i = 0; i < n; i++) ctx->sk_lwe[i] = w[i] & 1;
    rand_words(ctx->rkey, stream_id(DOM_SK_GLWE, 0), 0, w.data(), D);
    for (uint32_t i = 0; i < D; i++) ctx->sk_glwe[i] = w[i] & 1;
}

// support of each GLWE key polynomial (binary key => A*S is a signed sum of shifted copies of A)
static std::vector<std::vector<uint32_t>> glwe_support(const fbs_ctx *ctx) {
    std::vector<std::vector<uint32_t>> support(ctx->p.k);
    for (uint32_t c = 0; c < ctx->p.k; c++)
        for (uint32_t i = 0; i < ctx->N; i++)
            if (ctx->sk_glwe[(size_t)c * ctx->N + i]) support[c].push_back(i);
    return support;
}

// the bit GGSW sample g encrypts: key bit g, or for pairs (s0, s1) of key bits the products s0(1-s1), (1-s0)s1, s0 s1
static uint64_t ggsw_bit(const fbs_ctx *ctx, size_t g) {
    if (ctx->group != 2) return ctx->sk_lwe[g];
    const uint64_t s0 = ctx->sk_lwe[2 * (g / 3)], s1 = ctx->sk_lwe[2 * (g / 3) + 1];
    return g % 3 == 0 ? (s0 & (1 - s1)) : g % 3 == 1 ? ((1 - s0) & s1) : (s0 & s1);
}

void host_keygen(fbs_ctx *ctx) {
    const fbs_params &p = ctx->p;
    const uint32_t N = ctx->N, D = ctx->D, n = p.n, k = p.k, l = p.l_bsk, t = p.t_ksk, rows = ctx->rows;
    draw_secrets(ctx);
    const std::vector<std::vector<uint32_t>> support = glwe_support(ctx);
    const size_t row_words = (size_t)(k + 1) * N;
    ctx->bsk.assign(ctx->n_ggsw * rows * row_words, 0);
    parallel_for(ctx->n_ggsw * rows, [&](size_t r0, size_t r1) {
        for (size_t r = r0; r < r1; r++) {
            const uint32_t rr = (uint32_t)(r % rows), comp = rr / l, lv = rr % l;
            uint64_t *row = ctx->bsk.data() + r * row_words;
            glwe_zero_sample(ctx->rkey, stream_id(DOM_BSK_MASK, r), ctx->rkey, stream_id(DOM_BSK_NOISE, r), p.sigma_glwe, p.sampler,
                             support, N, row, row + (size_t)k * N);
            if (ggsw_bit(ctx, r / rows)) row[(size_t)comp * N] = fq_add(row[(size_t)comp * N], ctx->g[lv]);
        }
    });

    ctx->ksk.assign((size_t)D * t * (n + 1), 0);
    parallel_for((size_t)D * t, [&](size_t r0, size_t r1) {
        for (size_t r = r0; r < r1; r++) {
            uint64_t *row = ctx->ksk.data() + r * (n + 1);
            mask_words(ctx->rkey, stream_id(DOM_KSK_MASK, r), 0, row, n);
            row[n] = lwe_body(ctx->rkey, stream_id(DOM_KSK_NOISE, r), p.sigma_lwe, p.sampler, row, ctx->sk_lwe.data(), n);
            if (ctx->sk_glwe[r / t]) row[n] = fq_add(row[n], ctx->h[r % t]);
        }
    });
}

// ---------------------------------------------------------------------------------------------
// seeded keys: every mask under the public mask key, so that only the bodies travel
// ---------------------------------------------------------------------------------------------
RandKey mask_key_of(const RandKey &key) {
    uint64_t blk[8];
    chacha_block(key.w, stream_id(DOM_MASK_KEY, 0), 0, blk);
    RandKey m;
    for (int i = 0; i < 4; i++) {
        m.w[2 * i] = (uint32_t)blk[i];
        m.w[2 * i + 1] = (uint32_t)(blk[i] >> 32);
    }
    return m;
}

// Row r of the bootstrapping key, r = g (k+1) l + comp l + lv: mask A_c = fold(words c N .. c N + N - 1 of stream
// (DOM_SBSK_MASK, r)) under the mask key, body = e + sum_c A_c S_c + the message, e on stream (DOM_SBSK_NOISE, r) under the
// context key.  The message sits in the body whatever the component: bit g_lv at X^0 for comp = k, -bit g_lv S_comp for a mask
// row.  That is the phase fbs_keygen's rows have (its g_lv sits on A_comp), and the same distribution --
// the server, which regenerates the masks, needs no secret bit.  Key-switching row r = (j, v): mask = fold(stream
// (DOM_SKSK_MASK, r)), body = e + <a, sk_lwe> + sk_glwe[j] h_v.
void host_keygen_seeded(fbs_ctx *ctx) {
    const fbs_params &p = ctx->p;
    const uint32_t N = ctx->N, D = ctx->D, n = p.n, k = p.k, l = p.l_bsk, t = p.t_ksk, rows = ctx->rows;
    draw_secrets(ctx);
    ctx->mask_key = mask_key_of(ctx->rkey);
    const std::vector<std::vector<uint32_t>> support = glwe_support(ctx);
    std::vector<uint64_t> bsk_bodies(ctx->n_ggsw * rows * N), ksk_bodies((size_t)D * t);
    parallel_for(ctx->n_ggsw * rows, [&](size_t r0, size_t r1) {
        std::vector<uint64_t> a((size_t)k * N);
        for (size_t r = r0; r < r1; r++) {
            const size_t g = r / rows;
            const uint32_t rr = (uint32_t)(r % rows), comp = rr / l, lv = rr % l;
            uint64_t *body = bsk_bodies.data() + r * N;
            glwe_zero_sample(ctx->mask_key, stream_id(DOM_SBSK_MASK, r), ctx->rkey, stream_id(DOM_SBSK_NOISE, r), p.sigma_glwe, p.sampler,
                             support, N, a.data(), body);
            if (!ggsw_bit(ctx, g)) continue;
            if (comp == k) {
                body[0] = fq_add(body[0], ctx->g[lv]);
            } else {
                for (uint32_t j : support[comp]) body[j] = fq_sub(body[j], ctx->g[lv]);
            }
        }
    });
    parallel_for((size_t)D * t, [&](size_t r0, size_t r1) {
        std::vector<uint64_t> a(n);
        for (size_t r = r0; r < r1; r++) {
            mask_words(ctx->mask_key, stream_id(DOM_SKSK_MASK, r), 0, a.data(), n);
            ksk_bodies[r] = lwe_body(ctx->rkey, stream_id(DOM_SKSK_NOISE, r), p.sigma_lwe, p.sampler, a.data(), ctx->sk_lwe.data(), n);
            if (ctx->sk_glwe[r / t]) ksk_bodies[r] = fq_add(ksk_bodies[r], ctx->h[r % t]);
        }
    });
    host_expand_seeded_keys(ctx, ctx->mask_key, bsk_bodies.data(), ksk_bodies.data(), ctx->bsk, ctx->ksk);
}

void host_expand_seeded_keys(const fbs_ctx *ctx, const RandKey &mask_key, const uint64_t *bsk_bodies, const uint64_t *ksk_bodies,
                             std::vector<uint64_t> &bsk, std::vector<uint64_t> &ksk) {
    const uint32_t N = ctx->N, D = ctx->D, n = ctx->p.n, k = ctx->p.k, t = ctx->p.t_ksk, rows = ctx->rows;
    const size_t row_words = (size_t)(k + 1) * N;
    bsk.assign(ctx->n_ggsw * rows * row_words, 0);
    parallel_for(ctx->n_ggsw * rows, [&](size_t r0, size_t r1) {
        for (size_t r = r0; r < r1; r++) {
            uint64_t *row = bsk.data() + r * row_words;
            mask_words(mask_key, stream_id(DOM_SBSK_MASK, r), 0, row, (size_t)k * N);   // the k columns are one run of the stream
            std::memcpy(row + (size_t)k * N, bsk_bodies + r * N, (size_t)N * 8);
        }
    });
    ksk.assign((size_t)D * t * (n + 1), 0);
    parallel_for((size_t)D * t, [&](size_t r0, size_t r1) {
        for (size_t r = r0; r < r1; r++) {
            uint64_t *row = ksk.data() + r * (n + 1);
            mask_words(mask_key, stream_id(DOM_SKSK_MASK, r), 0, row, n);
            row[n] = ksk_bodies[r];
        }
    });
}

void host_encrypt_seeded(const fbs_ctx *ctx, const int64_t *msgs, size_t count, uint64_t nonce0, uint64_t *bodies) {
    const uint32_t D = ctx->D;
    const uint64_t delta = 2 * ctx->delta_half;
    parallel_for(count, [&](size_t a, size_t b) {
        std::vector<uint64_t> mask(D);
        for (size_t i = a; i < b; i++) {
            mask_words(ctx->mask_key, stream_id(DOM_SENC_MASK, nonce0 + i), 0, mask.data(), D);
            const uint64_t body = lwe_body(ctx->rkey, stream_id(DOM_SENC_NOISE, nonce0 + i), ctx->p.sigma_glwe, ctx->p.sampler, mask.data(),
                                           ctx->sk_glwe.data(), D);
            bodies[i] = fq_add(body, fq_mul(fq_from_i64(msgs[i]), delta));
        }
    });
}

void host_expand_seeded(const fbs_ctx *ctx, const uint64_t *bodies, size_t count, uint64_t nonce0, uint64_t *cts) {
    const uint32_t D = ctx->D;
    parallel_for(count, [&](size_t a, size_t b) {
        for (size_t i = a; i < b; i++) {
            uint64_t *ct = cts + i * (D + 1);
            mask_words(ctx->mask_key, stream_id(DOM_SENC_MASK, nonce0 + i), 0, ct, D);
            ct[D] = bodies[i];
        }
    });
}

// Do the evaluation keys decrypt under the secrets they came with?  A handful of GGSW samples (every row) and key-switching rows,
// each phase compared with what the layout of fbs_key_sizes says it encrypts: a key in another sample / row / column order has
// uniform phases and fails here instead of bootstrapping to garbage.  Tolerance: 16 standard deviations of the set's noise.
const char *imported_keys_mismatch(const fbs_ctx *ctx, const uint64_t *sk_lwe, const uint64_t *sk_glwe, const uint64_t *bsk,
                                   const uint64_t *ksk) {
    const fbs_params &p = ctx->p;
    const uint32_t N = ctx->N, D = ctx->D, n = p.n, k = p.k, l = p.l_bsk, t = p.t_ksk, rows = ctx->rows;
    auto far = [](uint64_t got, uint64_t want, double tol) { return std::fabs(fq_centered(fq_sub(got, want))) > tol; };
    const double tol_glwe = 1024.0 + 16.0 * (double)p.sigma_glwe, tol_lwe = 1024.0 + 16.0 * (double)p.sigma_lwe;
    std::vector<size_t> samples = {0, 1, 2, ctx->n_ggsw / 2, ctx->n_ggsw - 1};
    std::vector<uint64_t> phase(N);
    for (size_t g : samples) {
        if (g >= ctx->n_ggsw) continue;
        uint64_t bit;
        if (ctx->group == 2) {   // sample g of 3n/2 encrypts a product of the key bits 2 (g / 3) and 2 (g / 3) + 1
            const uint64_t s0 = sk_lwe[2 * (g / 3)], s1 = sk_lwe[2 * (g / 3) + 1];
            bit = g % 3 == 0 ? (s0 & (1 - s1)) : g % 3 == 1 ? ((1 - s0) & s1) : (s0 & s1);
        } else {
            bit = sk_lwe[g];
        }
        for (uint32_t rr = 0; rr < rows; rr++) {
            const uint32_t comp = rr / l, lv = rr % l;
            const uint64_t *row = bsk + (g * rows + rr) * (size_t)(k + 1) * N;
            for (uint32_t j = 0; j < N; j++) phase[j] = row[(size_t)k * N + j];
            for (uint32_t c = 0; c < k; c++)                            // phase -= A_c * S_c (negacyclic, binary S)
                for (uint32_t sh = 0; sh < N; sh++) {
                    if (!sk_glwe[(size_t)c * N + sh]) continue;
                    const uint64_t *a = row + (size_t)c * N;
                    for (uint32_t j = 0; j < N - sh; j++) phase[j + sh] = fq_sub(phase[j + sh], a[j]);
                    for (uint32_t j = N - sh; j < N; j++) phase[j + sh - N] = fq_add(phase[j + sh - N], a[j]);
                }
            // row (comp, lv) = GLWE(0) + bit g_lv on component comp: the phase is bit g_lv at X^0 (body row), -bit g_lv S_comp (mask rows)
            for (uint32_t j = 0; j < N; j++) {
                uint64_t want = 0;
                if (bit && comp == k && j == 0) want = ctx->g[lv];
                if (bit && comp < k && sk_glwe[(size_t)comp * N + j]) want = fq_sub(0, ctx->g[lv]);
                if (far(phase[j], want, tol_glwe)) return "bootstrapping key does not decrypt under the supplied secrets (sample / row / column order of fbs_key_sizes?)";
            }
        }
    }
    const size_t ksk_rows = (size_t)D * t;
    for (size_t r : {(size_t)0, (size_t)1, (size_t)2, (size_t)3, ksk_rows / 2, ksk_rows - 4, ksk_rows - 3, ksk_rows - 2, ksk_rows - 1}) {
        if (r >= ksk_rows) continue;
        const uint32_t j = (uint32_t)(r / t), v = (uint32_t)(r % t);
        const uint64_t *row = ksk + r * (size_t)(n + 1);
        uint64_t ph = row[n];
        for (uint32_t i = 0; i < n; i++)
            if (sk_lwe[i]) ph = fq_sub(ph, row[i]);
        if (far(ph, sk_glwe[j] ? ctx->h[v] : 0, tol_lwe)) return "key-switching key does not decrypt under the supplied secrets (row order [kN][t][n+1]?)";
    }
    return nullptr;
}

// ---------------------------------------------------------------------------------------------
// encrypt / decrypt under the big key
// ---------------------------------------------------------------------------------------------
void host_encrypt(const fbs_ctx *ctx, const int64_t *msgs, size_t count, uint64_t nonce0, uint64_t *cts) {
    const uint32_t D = ctx->D;
    const uint64_t delta = 2 * ctx->delta_half;
    parallel_for(count, [&](size_t a, size_t b) {
        for (size_t i = a; i < b; i++) {
            uint64_t *ct = cts + i * (D + 1);
            mask_words(ctx->rkey, stream_id(DOM_ENC_MASK, nonce0 + i), 0, ct, D);
            const uint64_t body = lwe_body(ctx->rkey, stream_id(DOM_ENC_NOISE, nonce0 + i), ctx->p.sigma_glwe, ctx->p.sampler, ct,
                                           ctx->sk_glwe.data(), D);
            ct[D] = fq_add(body, fq_mul(fq_from_i64(msgs[i]), delta));
        }
    });
}

void host_decrypt(const fbs_ctx *ctx, const uint64_t *cts, size_t count, int64_t *msgs) {
    const uint32_t D = ctx->D;
    const uint64_t two_p = 2ull * ctx->p.p_msg;
    parallel_for(count, [&](size_t a, size_t b) {
        for (size_t i = a; i < b; i++) {
            const uint64_t *ct = cts + i * (D + 1);
            uint64_t phase = ct[D];
            for (uint32_t j = 0; j < D; j++)
                if (ctx->sk_glwe[j]) phase = fq_sub(phase, ct[j]);
            unsigned __int128 v = (unsigned __int128)phase * two_p + FQ / 2;
            msgs[i] = (int64_t)((uint64_t)(v / FQ) % two_p);
        }
    });
}

// Compact outputs (fbs_compact.hpp): the phase of the packed fields under the small key, rounded to a message
void host_decrypt_compact(const fbs_ctx *ctx, const uint64_t *words, size_t count, uint32_t bits, int64_t *msgs) {
    const uint32_t n = ctx->p.n, W = compact_words(n, bits);
    const uint64_t two_p = 2ull * ctx->p.p_msg;
    parallel_for(count, [&](size_t a, size_t b) {
        for (size_t c = a; c < b; c++) {
            const uint64_t *ct = words + c * W;
            uint32_t sum = 0;
            for (uint32_t i = 0; i < n; i++)
                if (ctx->sk_lwe[i]) sum += compact_field(ct, i, bits);
            msgs[c] = compact_decode(compact_field(ct, n, bits), sum, bits, two_p);
        }
    });
}

void host_compact_trivial(const fbs_ctx *ctx, uint64_t body, uint32_t bits, uint64_t *words) {
    const uint32_t n = ctx->p.n, W = compact_words(n, bits), m_n = compact_round(body, bits);
    for (uint32_t j = 0; j < W; j++) words[j] = compact_word(j, n + 1, bits, [&](uint32_t f) { return f == n ? m_n : 0u; });
}

// ---------------------------------------------------------------------------------------------
// Packed outputs (fbs_pack.hpp; include/fbs_exec.h, "packed outputs") and folded state.  The gadget keys (GadgetKind,
// fbs_internal.hpp): GLWE encryptions under the big key of the constants src[i] h_v, masks under the public mask key and noise
// under the context's key, each on streams of the kind's own -- made only when asked for, so that nothing else a context
// derives changes.
// ---------------------------------------------------------------------------------------------
// bodies [rows][t][N] of the rows (i, v): a GLWE zero sample on the kind's streams (mask_dom, r), (noise_dom, r), r = i t + v, plus
// src[i] h_v at X^0 -- the packing key's rows (src = sk_lwe) and the fold key's (src = sk_glwe)
void host_gadget_keygen(const fbs_ctx *ctx, GadgetKind kind, uint32_t t, uint32_t gamma, std::vector<uint64_t> &bodies) {
    const uint32_t N = ctx->N, k = ctx->p.k;
    const GadgetKindInfo &gk = GADGET_KINDS[kind];
    const std::vector<uint64_t> &src = gadget_secret(*ctx, kind);
    const std::vector<std::vector<uint32_t>> support = glwe_support(ctx);
    bodies.assign(src.size() * t * N, 0);
    parallel_for(src.size() * t, [&](size_t r0, size_t r1) {
        std::vector<uint64_t> a((size_t)k * N);
        for (size_t r = r0; r < r1; r++) {
            const size_t i = r / t;
            const uint32_t v = (uint32_t)(r % t);
            uint64_t *body = bodies.data() + r * N;
            glwe_zero_sample(ctx->mask_key, stream_id(gk.mask_dom, r), ctx->rkey, stream_id(gk.noise_dom, r), ctx->p.sigma_glwe,
                             ctx->p.sampler, support, N, a.data(), body);
            if (src[i]) body[0] = fq_add(body[0], pack_gadget(gamma, v));
        }
    });
}
// (mask key, bodies [rows t][N]) -> the whole rows [rows t][k+1][N]
void host_expand_gadget_key(const fbs_ctx *ctx, GadgetKind kind, const RandKey &mask_key, uint32_t t, const uint64_t *bodies,
                            std::vector<uint64_t> &full) {
    const uint32_t N = ctx->N, k = ctx->p.k;
    const size_t rows = (size_t)gadget_rows(*ctx, kind) * t, row_words = (size_t)(k + 1) * N;
    full.assign(rows * row_words, 0);
    parallel_for(rows, [&](size_t r0, size_t r1) {
        for (size_t r = r0; r < r1; r++) {
            uint64_t *row = full.data() + r * row_words;
            mask_words(mask_key, stream_id(GADGET_KINDS[kind].mask_dom, r), 0, row, (size_t)k * N);
            std::memcpy(row + (size_t)k * N, bodies + r * N, (size_t)N * 8);
        }
    });
}

// The decode: phase_j = body_j - sum_c (A_c S_c)_j mod 2^w over the fields of each sample (32-bit wrapping sums are exact mod 2^w),
// msg = round(phase 2p / 2^w) mod 2p.  Sample g holds outputs g N .. g N + fill - 1 in its first `fill` coefficients.
void host_decrypt_packed(const fbs_ctx *ctx, const uint64_t *words, size_t count, uint32_t bits, int64_t *msgs) {
    const uint32_t N = ctx->N, k = ctx->p.k;
    const uint64_t two_p = 2ull * ctx->p.p_msg;
    const size_t samples = (count + N - 1) / N, full_words = packed_sample_words(k, N, N, bits);
    const std::vector<std::vector<uint32_t>> support = glwe_support(ctx);
    parallel_for(samples, [&](size_t g0, size_t g1) {
        std::vector<uint32_t> sum(N), a(N);
        for (size_t g = g0; g < g1; g++) {
            const uint64_t *sample = words + g * full_words;
            const uint32_t fill = (uint32_t)std::min<size_t>(N, count - g * N);
            std::fill(sum.begin(), sum.end(), 0u);
            for (uint32_t c = 0; c < k; c++) {
                for (uint32_t j = 0; j < N; j++) a[j] = compact_field(sample, c * N + j, bits);
                for (uint32_t sh : support[c]) {   // sum += X^sh A_c
                    for (uint32_t j = 0; j < N - sh; j++) sum[j + sh] += a[j];
                    for (uint32_t j = N - sh; j < N; j++) sum[j + sh - N] -= a[j];
                }
            }
            for (uint32_t j = 0; j < fill; j++)
                msgs[g * N + j] = compact_decode(compact_field(sample, k * N + j, bits), sum[j], bits, two_p);
        }
    });
}

// ---------------------------------------------------------------------------------------------
// test vector for one table.  A table longer than p is only computable when the values met at
// x and x+p add up to one constant c (the reference's three "modes", map_to_fbs.py:81-98 are
// c = 1, 0, 2): then f - c/2 is negacyclic, the polynomial carries (2f - c) * Delta/2 and c*Delta/2
// is added back after sample extraction.
// ---------------------------------------------------------------------------------------------
int host_build_tv(const fbs_ctx *ctx, const int32_t *table, uint32_t len, uint64_t *tv, uint64_t *post_add) {
    const uint32_t p = ctx->p.p_msg, N = ctx->N;
    if (len == 0 || len > 2 * p) return FBS_E_TABLE;
    int64_t c = 0;
    if (len > p) {
        c = (int64_t)table[0] + table[p];
        for (uint32_t i = 0; i + p < len; i++)
            if ((int64_t)table[i] + table[i + p] != c) return FBS_E_TABLE;
    }
    std::vector<uint64_t> enc(p);
    for (uint32_t x = 0; x < p; x++) {
        int64_t f = x < len ? table[x] : 0;   // unreachable slots
        enc[x] = fq_mul(fq_from_i64(2 * f - c), ctx->delta_half);
    }
    for (uint32_t j = 0; j < N; j++) {
        uint64_t x = ((uint64_t)j * 2 * p + N) / (2ull * N);   // nearest multiple of N/p
        tv[j] = x < p ? enc[x] : fq_neg(enc[0]);               // the half box below X^N wraps to -f(0)
    }
    *post_add = fq_mul(fq_from_i64(c), ctx->delta_half);
    return FBS_OK;
}

// The box rule above as the map of a mapped fold (fbs_lookup_map of include/fbs_exec.h, "encrypted-index reads"): coefficient j takes
// source base + slot stride for slot < len, nothing for len <= slot < p, and source `base` negated in the half box below X^N.
// Pure: no context.  A source index must fit the 31 bits a map entry has for it.
int host_lookup_map(uint32_t p, uint32_t N, uint32_t len, uint32_t base, uint32_t stride, uint32_t *map_out) {
    if (!map_out) return FBS_E_INVALID;
    if (p < 2) return set_error(nullptr, FBS_E_INVALID, "a table needs p >= 2");
    if (N < 2 || N > (1u << 16) || (N & (N - 1))) return set_error(nullptr, FBS_E_INVALID, "N must be a power of two in [2, 2^16]");
    if (len == 0) return set_error(nullptr, FBS_E_INVALID, "a table has at least one entry");
    if (len > p) return set_error(nullptr, FBS_E_INVALID, "a table has at most p entries");
    if ((uint64_t)base + (uint64_t)(len - 1) * stride >= FOLD_MAP_NEG) return set_error(nullptr, FBS_E_INVALID, "a source index must stay below 2^31");
    for (uint32_t j = 0; j < N; j++) {
        const uint64_t x = ((uint64_t)j * 2 * p + N) / (2ull * N);
        map_out[j] = x < len ? base + (uint32_t)x * stride : x < p ? FOLD_MAP_NONE : base | FOLD_MAP_NEG;
    }
    return FBS_OK;
}

// The map of a WRITABLE table (fbs_table_map of include/fbs_exec.h, "encrypted tables"): an entry takes `spread` ordinary boxes, the
// wide slot of a signed position c in (-N, N) being W(c) = floor((2 p c + s N) / (2 s N)).  Coefficient j takes source
// base + W(j) stride for W(j) < len, source `base` negated where W(j - N) == 0 (2 p (N - j) <= s N: the half box of entry 0 below
// X^N), nothing elsewhere.  The two cases never meet: below X^N, W(j) >= floor(p / s) >= len.  spread = 1 is host_lookup_map.
int host_table_map(uint32_t p, uint32_t N, uint32_t spread, uint32_t len, uint32_t base, uint32_t stride, uint32_t *map_out) {
    if (!map_out) return FBS_E_INVALID;
    if (p < 2) return set_error(nullptr, FBS_E_INVALID, "a table needs p >= 2");
    if (N < 2 || N > (1u << 16) || (N & (N - 1))) return set_error(nullptr, FBS_E_INVALID, "N must be a power of two in [2, 2^16]");
    if (spread < 1) return set_error(nullptr, FBS_E_INVALID, "an entry takes at least one box");
    if (len == 0) return set_error(nullptr, FBS_E_INVALID, "a table has at least one entry");
    if (len > p / spread) return set_error(nullptr, FBS_E_INVALID, "a table has at most floor(p / spread) entries");
    if ((uint64_t)base + (uint64_t)(len - 1) * stride >= FOLD_MAP_NEG) return set_error(nullptr, FBS_E_INVALID, "a source index must stay below 2^31");
    const uint64_t sN = (uint64_t)spread * N;
    for (uint32_t j = 0; j < N; j++) {
        const uint64_t w = ((uint64_t)j * 2 * p + sN) / (2 * sN);
        map_out[j] = w < len ? base + (uint32_t)w * stride : (uint64_t)(N - j) * 2 * p <= sN ? base | FOLD_MAP_NEG : FOLD_MAP_NONE;
    }
    return FBS_OK;
}

// ---------------------------------------------------------------------------------------------
// Several tables on one blind rotation (multi-value bootstrap; Carpov, Izabachene, Mollimard, CT-RSA 2019).  The test
// vector above is delta_half * G(X) with G_j = +-(2 f - c), and (1 + X + .. + X^(N-1)) (1 - X) = 2 in Z[X]/(X^N + 1), so
//     TV_F = TV_0 * D_F,   TV_0 = delta_half (1 + X + .. + X^(N-1)),   D_F = G (1 - X) / 2
// -- an integer polynomial (every G_j has the parity of c) that is non-zero only where the table changes value: at box
// boundaries j with f(x_j) != f(x_j - 1), and where the last half box flips to -(2 f(0) - c).  The coefficient at j = 0,
// G_0 + G_(N-1), is zero by that very flip.
// ---------------------------------------------------------------------------------------------
int host_build_tv_diff(const fbs_ctx *ctx, const int32_t *table, uint32_t len, uint32_t *pos, int32_t *val, uint32_t *count,
                       uint64_t *norm2, uint64_t *g_norm2, uint64_t *abs_sum) {
    const uint32_t p = ctx->p.p_msg, N = ctx->N;
    if (len == 0 || len > 2 * p) return FBS_E_TABLE;
    int64_t c = 0;
    if (len > p) {
        c = (int64_t)table[0] + table[p];
        for (uint32_t i = 0; i + p < len; i++)
            if ((int64_t)table[i] + table[i + p] != c) return FBS_E_TABLE;
    }
    auto g_of = [&](uint32_t j) -> int64_t {
        const uint64_t x = ((uint64_t)j * 2 * p + N) / (2ull * N);
        const int64_t f = x < p ? (x < len ? table[x] : 0) : table[0];
        return x < p ? 2 * f - c : -(2 * f - c);
    };
    uint32_t n = 0;
    uint64_t n2 = 0, g2 = 0, sum = 0;
    int64_t prev = -g_of(N - 1);   // G_(-1) = -G_(N-1)
    for (uint32_t j = 0; j < N; j++) {
        const int64_t g = g_of(j);
        g2 += (uint64_t)(g * g);
        const int64_t d = (g - prev) / 2;
        prev = g;
        if (d == 0) continue;
        if (n > p || d > INT32_MAX || d < INT32_MIN) return FBS_E_TABLE;   // (cannot happen: p boxes, p + 1 boundaries)
        pos[n] = j;
        val[n] = (int32_t)d;
        n++;
        n2 += (uint64_t)(d * d);
        sum += (uint64_t)(d < 0 ? -d : d);
    }
    *count = n;
    *norm2 = n2;
    *g_norm2 = g2;
    *abs_sum = sum;
    return FBS_OK;
}

// ---------------------------------------------------------------------------------------------
// twiddles for the merged negacyclic NTT: fwd[i] = psi^bitrev(i), inv[i] = psi^-bitrev(i), psi = 7^((q-1)/2N)
// (any primitive 2N-th root gives the same ciphertexts: the transform is an internal representation).
// Entries [N, 2N) repeat the two half-size subtrees (nodes 2 and 3 of the twiddle tree) as tables of their own, N/2
// entries each: entry i of half h = entry ((2 + h) << d) + (i - 2^d), d = floor(log2 i); entries [2N, 3N) the four
// quarter-size subtrees (nodes 4 .. 7) likewise -- what the multi-wave transforms (WavesNtt, fbs_ntt_split.hpp) gather from.
// Two more forward entries follow (tw_table_words, fbs_field.hpp): tw[1] tw[2] and tw[1] tw[3], for the fused opening of the
// digit transforms (SplitNtt::first_two_stages).
// ---------------------------------------------------------------------------------------------
void host_twiddles(uint32_t log_n, std::vector<uint64_t> &fwd, std::vector<uint64_t> &inv) {
    const uint32_t N = 1u << log_n;
    const uint64_t psi = fq_pow(FQ_GENERATOR, (FQ - 1) / (2ull * N));
    const uint64_t psi_inv = fq_inv(psi);
    fwd.assign(N, 1);
    inv.assign(N, 1);
    for (uint32_t i = 1; i < N; i++) {
        uint32_t r = 0;
        for (uint32_t b = 0; b < log_n; b++) r |= ((i >> b) & 1u) << (log_n - 1 - b);
        fwd[i] = fq_pow(psi, r);
        inv[i] = fq_pow(psi_inv, r);
    }
    fwd.resize(3 * (size_t)N, 1);
    inv.resize(3 * (size_t)N, 1);
    for (uint32_t parts = 2, base = N; parts <= 4; parts *= 2, base += N)   // [N, 2N): the two halves; [2N, 3N): the four quarters
        for (uint32_t h = 0; h < parts; h++)
            for (uint32_t i = 1; i < N / parts; i++) {
                uint32_t d = 31 - (uint32_t)__builtin_clz(i);
                uint32_t big = ((parts + h) << d) + (i - (1u << d));
                fwd[base + h * (N / parts) + i] = fwd[big];
                inv[base + h * (N / parts) + i] = inv[big];
            }
    fwd.resize(tw_table_words(N), 1);   // the fused opening's products (tw_fused_word); the inverse table keeps the same size
    inv.resize(tw_table_words(N), 1);
    fwd[tw_fused_word(N)] = fq_mul(fwd[1], fwd[2]);
    fwd[tw_fused_word(N) + 1] = fq_mul(fwd[1], fwd[3]);
}

}  // namespace fbs

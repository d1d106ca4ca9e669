// Public-key inputs (include/fbs_exec.h, "public-key inputs"): a data owner who holds neither the secret key nor the GPU encrypts
// under a public key the key holder published; the server turns the GLWE samples into big-key ciphertexts by sample extraction.
// Host code with no device in it, compiled into libfbsexec.so and, with FBS_HOST_ONLY, into libfbspublic.so (make public), which
// exports these entries and nothing else.  The device side of the expansion is fbs_public.hip; its two entries are in fbs_capi.cpp.
//
//   public key     masks A[r][c] = fold(words c N .. c N + N - 1 of stream (DOM_PUB_MASK, r)) under the public mask key,
//                  bodies P_r = sum_c A[r][c] S_c + E_r, E_r = samples 0 .. N - 1 of stream (DOM_PUB_NOISE, r) under the noise seed
//   encryption     sample nu: u_r from the bits of stream (DOM_PUB_ENC_U, nu), e_c = samples c N .. of stream (DOM_PUB_ENC_NOISE, nu),
//                  both under the encryptor's key; A'_c = sum_r u_r A[r][c] + e_c, B' = sum_r u_r P_r + e_k + Delta M
//   expansion      word c N + i of message t's ciphertext = A'_c[t - i] (i <= t), -A'_c[N + t - i] (i > t); word k N = B'[t]
// Every product is by a binary polynomial: a signed sum of shifted copies (add_times_key, fbs_host.cpp), as the key generation does it.
#include <algorithm>
#include <atomic>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "fbs_api_checks.hpp"
#include "fbs_internal.hpp"

using namespace fbs;

struct fbs_pub {
    fbs_params p{};
    uint32_t N = 0, k = 0;
    uint64_t delta = 0;                // 2 round(q / 4p)
    RandKey key{};                     // the encryptor's own: u and e of every sample are expanded from it
    std::vector<uint64_t> a;           // [k][k][N]: A[r][c], regenerated from the mask key
    std::vector<uint64_t> bodies;      // [k][N]: P_r
    mutable std::atomic<uint64_t> next_nonce{1ull << 55};   // fresh streams: [2^55, 2^56), as a context's
    mutable std::string err;
};

namespace fbs {

size_t first_noncanonical(const uint64_t *w, size_t words) {
    for (size_t i = 0; i < words; i++)
        if (w[i] >= FQ) return i;
    return words;
}

void host_pub_expand(uint32_t k, uint32_t N, const uint64_t *glwe, size_t count, uint64_t *cts) {
    const size_t D = (size_t)k * N;
    for (size_t j = 0; j < count; j++) {
        const uint64_t *sample = glwe + (j / N) * (D + N);
        const uint32_t t = (uint32_t)(j % N);
        uint64_t *ct = cts + j * (D + 1);
        for (uint32_t c = 0; c < k; c++) {
            const uint64_t *a = sample + (size_t)c * N;
            for (uint32_t i = 0; i <= t; i++) ct[(size_t)c * N + i] = a[t - i];
            for (uint32_t i = t + 1; i < N; i++) ct[(size_t)c * N + i] = fq_neg(a[N + t - i]);
        }
        ct[D] = sample[D + t];
    }
}

}  // namespace fbs

namespace {

int pub_fail(const fbs_pub *pub, int code, const std::string &msg) {
    if (pub) pub->err = msg;
    else set_error(nullptr, code, msg);
    return code;
}

// what the entries without a handle need of a parameter set, after the admission a context applies (params_admitted)
struct Shape {
    uint32_t N = 0, k = 0;
    uint64_t delta = 0;
};
int shape_of(const fbs_params *p, Shape &sh) {
    fbs_ctx *probe = nullptr;
    if (int rc = params_admitted(p, &probe)) return rc;
    std::unique_ptr<fbs_ctx> own(probe);
    sh.N = own->N;
    sh.k = own->p.k;
    sh.delta = 2 * own->delta_half;
    return FBS_OK;
}

RandKey key_of_bytes(const uint8_t b[32]) {
    RandKey k;
    for (int i = 0; i < 8; i++) k.w[i] = (uint32_t)b[4 * i] | (uint32_t)b[4 * i + 1] << 8 | (uint32_t)b[4 * i + 2] << 16 | (uint32_t)b[4 * i + 3] << 24;
    return k;
}

// A[r][c] for r, c < k -> a [k][k][N]
void draw_masks(const RandKey &mask_key, uint32_t k, uint32_t N, std::vector<uint64_t> &a) {
    a.resize((size_t)k * k * N);
    for (uint32_t r = 0; r < k; r++) mask_words(mask_key, stream_id(DOM_PUB_MASK, r), 0, a.data() + (size_t)r * k * N, (size_t)k * N);
}

size_t samples_of(size_t count, uint32_t N) { return count / N + (count % N ? 1 : 0); }

// G (k + 1) N words, or FBS_E_INVALID where they overflow
int sample_words(const fbs_pub *pub, uint32_t k, uint32_t N, size_t count, size_t *words) {
    const size_t G = samples_of(count, N), per = (size_t)(k + 1) * N;
    if (G > SIZE_MAX / 8 / per) return pub_fail(pub, FBS_E_INVALID, "the words of ceil(count / N) samples overflow");
    *words = G * per;
    return FBS_OK;
}

int check_messages(const fbs_pub *pub, const int64_t *msgs, size_t count) {
    const int64_t two_p = 2 * (int64_t)pub->p.p_msg;
    for (size_t i = 0; i < count; i++)
        if (msgs[i] < 0 || msgs[i] >= two_p) return pub_fail(pub, FBS_E_INVALID, "message " + std::to_string(i) + " is outside [0, 2p)");
    return FBS_OK;
}

void pub_encrypt(const fbs_pub *pub, const int64_t *msgs, size_t count, uint64_t nonce0, uint64_t *glwe) {
    const uint32_t N = pub->N, k = pub->k;
    const size_t D = (size_t)k * N, G = samples_of(count, N);
    std::vector<uint64_t> bits((D + 63) / 64);
    std::vector<std::vector<uint32_t>> support(k);
    for (size_t g = 0; g < G; g++) {
        const uint64_t nu = nonce0 + g;
        uint64_t *out = glwe + g * (D + N);
        rand_words(pub->key, stream_id(DOM_PUB_ENC_U, nu), 0, bits.data(), bits.size());
        for (uint32_t r = 0; r < k; r++) {
            support[r].clear();
            for (uint32_t j = 0; j < N; j++) {
                const size_t b = (size_t)r * N + j;
                if ((bits[b >> 6] >> (b & 63)) & 1) support[r].push_back(j);
            }
        }
        for (size_t i = 0; i < D + N; i++)
            out[i] = fq_from_i64(noise_sample(pub->key, stream_id(DOM_PUB_ENC_NOISE, nu), i, pub->p.sigma_glwe, pub->p.sampler));
        for (uint32_t r = 0; r < k; r++) {
            for (uint32_t c = 0; c < k; c++) add_times_key(out + (size_t)c * N, pub->a.data() + ((size_t)r * k + c) * N, support[r], N);
            add_times_key(out + D, pub->bodies.data() + (size_t)r * N, support[r], N);
        }
        const size_t fill = std::min<size_t>(N, count - g * N);
        for (size_t j = 0; j < fill; j++) out[D + j] = fq_add(out[D + j], fq_mul((uint64_t)msgs[g * N + j], pub->delta));
    }
}

}  // namespace

extern "C" {

int fbs_pub_key_words(const fbs_params *p, size_t *words) try {
    if (!words) return pub_fail(nullptr, FBS_E_INVALID, "null argument");
    Shape sh;
    if (int rc = shape_of(p, sh)) return rc;
    *words = (size_t)sh.k * sh.N;
    return FBS_OK;
} FBS_API_CATCH(nullptr)

int fbs_pub_keygen(const fbs_params *p, const uint8_t mask_key[32], const uint64_t *sk_glwe, const uint8_t noise_seed[32], uint64_t *bodies) try {
    if (!mask_key || !sk_glwe || !noise_seed || !bodies) return pub_fail(nullptr, FBS_E_INVALID, "null argument");
    Shape sh;
    if (int rc = shape_of(p, sh)) return rc;
    const uint32_t N = sh.N, k = sh.k;
    std::vector<std::vector<uint32_t>> support(k);
    for (uint32_t c = 0; c < k; c++)
        for (uint32_t j = 0; j < N; j++) {
            const uint64_t bit = sk_glwe[(size_t)c * N + j];
            if (bit > 1) return pub_fail(nullptr, FBS_E_INVALID, "secret keys are binary");
            if (bit) support[c].push_back(j);
        }
    std::vector<uint64_t> a((size_t)k * N), out((size_t)k * N);
    const RandKey masks = key_of_bytes(mask_key), noise = key_of_bytes(noise_seed);
    for (uint32_t r = 0; r < k; r++)   // row r: a GLWE zero sample; only its body travels
        glwe_zero_sample(masks, stream_id(DOM_PUB_MASK, r), noise, stream_id(DOM_PUB_NOISE, r), p->sigma_glwe, p->sampler, support, N,
                         a.data(), out.data() + (size_t)r * N);
    std::memcpy(bodies, out.data(), out.size() * 8);
    for (auto &s : support) std::fill(s.begin(), s.end(), 0u);   // (the secret's positions do not stay in freed memory)
    return FBS_OK;
} FBS_API_CATCH(nullptr)

int fbs_pub_create(const fbs_params *p, const uint8_t mask_key[32], const uint64_t *bodies, const uint8_t seed[32], fbs_pub **out) try {
    if (!out) return pub_fail(nullptr, FBS_E_INVALID, "null argument");
    *out = nullptr;
    if (!mask_key || !bodies || !seed) return pub_fail(nullptr, FBS_E_INVALID, "null argument");
    Shape sh;
    if (int rc = shape_of(p, sh)) return rc;
    const size_t words = (size_t)sh.k * sh.N, bad = first_noncanonical(bodies, words);
    if (bad < words) return pub_fail(nullptr, FBS_E_INVALID, "public-key word " + std::to_string(bad) + " is not a canonical residue");
    std::unique_ptr<fbs_pub> pub(new fbs_pub);
    pub->p = *p;
    pub->N = sh.N;
    pub->k = sh.k;
    pub->delta = sh.delta;
    pub->key = rand_key_derive(seed, *p);
    draw_masks(key_of_bytes(mask_key), sh.k, sh.N, pub->a);
    pub->bodies.assign(bodies, bodies + words);
    *out = pub.release();
    return FBS_OK;
} FBS_API_CATCH(nullptr)

void fbs_pub_destroy(fbs_pub *pub) try {
    if (!pub) return;
    std::memset(pub->key.w, 0, sizeof pub->key.w);   // u and e of every sample it made follow from this key
    delete pub;
} catch (...) {
}

const char *fbs_pub_last_error(const fbs_pub *pub) try {
    return pub ? pub->err.c_str() : create_error();
} catch (...) {
    return "";
}

int fbs_pub_words(const fbs_params *p, size_t count, size_t *words) try {
    if (!words) return pub_fail(nullptr, FBS_E_INVALID, "null argument");
    Shape sh;
    if (int rc = shape_of(p, sh)) return rc;
    return sample_words(nullptr, sh.k, sh.N, count, words);
} FBS_API_CATCH(nullptr)

int fbs_pub_encrypt(const fbs_pub *pub, const int64_t *msgs, size_t count, uint64_t nonce0, uint64_t *glwe) try {
    if (!pub || (count && (!msgs || !glwe))) return FBS_E_INVALID;
    const size_t G = samples_of(count, pub->N);
    if (nonce0 >= (1ull << 55) || G > (1ull << 55) - nonce0) return pub_fail(pub, FBS_E_INVALID, "nonce0 + samples must stay below 2^55");
    size_t words = 0;
    if (int rc = sample_words(pub, pub->k, pub->N, count, &words)) return rc;
    if (int rc = check_messages(pub, msgs, count)) return rc;
    pub_encrypt(pub, msgs, count, nonce0, glwe);
    return FBS_OK;
} catch (...) {
    return translate_exception([&](int, const char *text) { pub->err = text; });
}

int fbs_pub_encrypt_fresh(fbs_pub *pub, const int64_t *msgs, size_t count, uint64_t *glwe, uint64_t *nonce0) try {
    if (!pub || (count && (!msgs || !glwe))) return FBS_E_INVALID;
    const size_t G = samples_of(count, pub->N);
    const char *used_up = "encryption streams of this encryptor are used up";
    uint64_t first = pub->next_nonce.load(std::memory_order_relaxed);
    if (G > (1ull << 56) - first) return pub_fail(pub, FBS_E_STATE, used_up);   // (asked before anything else is checked: moves nothing)
    size_t words = 0;
    if (int rc = sample_words(pub, pub->k, pub->N, count, &words)) return rc;
    if (int rc = check_messages(pub, msgs, count)) return rc;
    do {   // reserved atomically, the bound checked before the counter moves: two threads never share a stream
        if (G > (1ull << 56) - first) return pub_fail(pub, FBS_E_STATE, used_up);
    } while (!pub->next_nonce.compare_exchange_weak(first, first + G, std::memory_order_relaxed));
    if (nonce0) *nonce0 = first;
    pub_encrypt(pub, msgs, count, first, glwe);
    return FBS_OK;
} catch (...) {
    return translate_exception([&](int, const char *text) { pub->err = text; });
}

int fbs_pub_expand(const fbs_params *p, const uint64_t *glwe, size_t count, uint64_t *cts) try {
    Shape sh;
    if (int rc = shape_of(p, sh)) return rc;
    if (count && (!glwe || !cts)) return pub_fail(nullptr, FBS_E_INVALID, "null argument");
    size_t words = 0;
    if (int rc = sample_words(nullptr, sh.k, sh.N, count, &words)) return rc;
    if (count > SIZE_MAX / 8 / ((size_t)sh.k * sh.N + 1)) return pub_fail(nullptr, FBS_E_INVALID, "count * (D + 1) words overflow");
    const size_t bad = first_noncanonical(glwe, words);
    if (bad < words) return pub_fail(nullptr, FBS_E_INVALID, "sample word " + std::to_string(bad) + " is not a canonical residue");
    host_pub_expand(sh.k, sh.N, glwe, count, cts);
    return FBS_OK;
} FBS_API_CATCH(nullptr)

}  // extern "C"

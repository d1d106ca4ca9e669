// Public-key inputs (include/fbs_exec.h, "public-key inputs") under AddressSanitizer and UBSan, as a program of its own: the host
// sources of libfbspublic.so compiled in, the C entries called as a C client calls them.  For the four toy sets of the Python
// tests -- k = 1 at N = 256 and N = 1024, k = 2 and k = 3 at N = 256 -- it makes a public key for a secret of its own, encrypts
// counts that leave the last sample partly filled (explicit and fresh streams), expands on the host and decrypts with the
// secret.  Every buffer is a heap block of exactly the size the word-count entries give: a word written or read past an end is a
// report.  The refusals run too: they must write nothing into blocks of size zero.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <vector>

#include "../../include/fbs_exec.h"

static const uint64_t Q = 0x3FFFFFF84001ull;
static int failures = 0;
#define CHECK(cond, ...)                          \
    do {                                          \
        if (!(cond)) {                            \
            std::printf("FAIL: " __VA_ARGS__);    \
            std::printf("\n");                    \
            failures++;                           \
        }                                         \
    } while (0)

static uint64_t splitmix(uint64_t &s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

template <class T>
static std::unique_ptr<T[]> block(size_t n) { return std::unique_ptr<T[]>(new T[n]); }   // exactly n elements, no slack

static fbs_params toy(uint32_t log_n, uint32_t k) {
    fbs_params p{};
    p.n = 12, p.log_n_poly = log_n, p.k = k, p.t_ksk = 8, p.gamma_ksk = 2, p.p_msg = 7, p.sigma_lwe = 1 << 8;
    if (k == 1) p.l_bsk = 3, p.beta_bsk = 7, p.sigma_glwe = 1 << 8, p.bsk_group = 1;
    else p.l_bsk = 1, p.beta_bsk = k == 2 ? 21 : 18, p.sigma_glwe = 4, p.bsk_group = 2;
    return p;
}

static int64_t decrypt(const uint64_t *ct, const uint64_t *sk, size_t D, uint32_t p_msg) {
    unsigned __int128 sum = 0;
    for (size_t j = 0; j < D; j++)
        if (sk[j]) sum += ct[j];
    const uint64_t phase = (uint64_t)(((unsigned __int128)ct[D] + (unsigned __int128)Q * D - sum) % Q);
    return (int64_t)((uint64_t)(((unsigned __int128)phase * 2 * p_msg + Q / 2) / Q) % (2 * p_msg));
}

static void run(const char *name, const fbs_params &p, uint32_t sampler) {
    fbs_params prm = p;
    prm.sampler = sampler;
    const size_t N = (size_t)1 << prm.log_n_poly, D = prm.k * N;
    uint64_t seed = 7 + prm.k * 1000 + N;
    uint8_t mask_key[32], noise_seed[32], enc_seed[32];
    for (int i = 0; i < 32; i++) mask_key[i] = (uint8_t)splitmix(seed), noise_seed[i] = (uint8_t)splitmix(seed), enc_seed[i] = (uint8_t)splitmix(seed);
    size_t key_words = 0;
    CHECK(fbs_pub_key_words(&prm, &key_words) == FBS_OK && key_words == D, "%s: key words", name);
    auto sk = block<uint64_t>(D);
    for (size_t j = 0; j < D; j++) sk[j] = splitmix(seed) & 1;
    auto bodies = block<uint64_t>(key_words);
    CHECK(fbs_pub_keygen(&prm, mask_key, sk.get(), noise_seed, bodies.get()) == FBS_OK, "%s: keygen: %s", name, fbs_pub_last_error(nullptr));
    fbs_pub *pub = nullptr;
    CHECK(fbs_pub_create(&prm, mask_key, bodies.get(), enc_seed, &pub) == FBS_OK && pub, "%s: create: %s", name, fbs_pub_last_error(nullptr));
    if (!pub) return;
    size_t checked = 0;
    for (size_t count : {(size_t)1, N - 1, N, N + 1, 2 * N + 3}) {
        for (int fresh = 0; fresh < 2; fresh++) {
            size_t words = 0;
            CHECK(fbs_pub_words(&prm, count, &words) == FBS_OK && words == (count + N - 1) / N * (prm.k + 1) * N, "%s: words of %zu", name, count);
            auto msgs = block<int64_t>(count);
            for (size_t i = 0; i < count; i++) msgs[i] = (int64_t)(splitmix(seed) % (2 * prm.p_msg));
            auto glwe = block<uint64_t>(words);
            uint64_t first = 0;
            const int rc = fresh ? fbs_pub_encrypt_fresh(pub, msgs.get(), count, glwe.get(), &first) : fbs_pub_encrypt(pub, msgs.get(), count, 1000 + count, glwe.get());
            CHECK(rc == FBS_OK, "%s: encrypt %zu: %s", name, count, fbs_pub_last_error(pub));
            CHECK(!fresh || first >= (1ull << 55), "%s: fresh stream %" PRIu64, name, first);
            for (size_t i = 0; i < words; i++) CHECK(glwe[i] < Q, "%s: word %zu not canonical", name, i);
            auto cts = block<uint64_t>(count * (D + 1));
            CHECK(fbs_pub_expand(&prm, glwe.get(), count, cts.get()) == FBS_OK, "%s: expand %zu: %s", name, count, fbs_pub_last_error(nullptr));
            for (size_t i = 0; i < count; i++, checked++)
                CHECK(decrypt(cts.get() + i * (D + 1), sk.get(), D, prm.p_msg) == msgs[i], "%s: message %zu of %zu", name, i, count);
        }
    }
    // refusals: nothing is written -- the destinations are blocks of no words at all
    auto none = block<uint64_t>(0);
    int64_t bad[2] = {0, 2 * (int64_t)prm.p_msg};
    CHECK(fbs_pub_encrypt(pub, bad, 2, 5, none.get()) == FBS_E_INVALID, "%s: message 2p", name);
    bad[1] = -1;
    CHECK(fbs_pub_encrypt_fresh(pub, bad, 2, none.get(), nullptr) == FBS_E_INVALID, "%s: message -1", name);
    bad[1] = 1;
    CHECK(fbs_pub_encrypt(pub, bad, 2, 1ull << 55, none.get()) == FBS_E_INVALID, "%s: nonce 2^55", name);
    CHECK(fbs_pub_encrypt(pub, bad, 0, 5, nullptr) == FBS_OK && fbs_pub_expand(&prm, nullptr, 0, nullptr) == FBS_OK, "%s: count 0", name);
    size_t words = 0;
    fbs_pub_words(&prm, 1, &words);
    auto glwe = block<uint64_t>(words);
    for (size_t i = 0; i < words; i++) glwe[i] = 0;
    glwe[words - 1] = Q;
    CHECK(fbs_pub_expand(&prm, glwe.get(), 1, none.get()) == FBS_E_INVALID, "%s: non-canonical last word", name);
    bodies[key_words - 1] = ~0ull;
    fbs_pub *other = nullptr;
    CHECK(fbs_pub_create(&prm, mask_key, bodies.get(), enc_seed, &other) == FBS_E_INVALID && !other, "%s: non-canonical body", name);
    fbs_pub_destroy(pub);
    fbs_pub_destroy(nullptr);
    std::printf("%s sampler %u: %zu messages\n", name, sampler, checked);
}

int main() {
    run("k1_N256", toy(8, 1), 0);
    run("k1_N1024", toy(10, 1), 0);
    run("k2_N256", toy(8, 2), 0);
    run("k3_N256", toy(8, 3), 0);
    run("k1_N256", toy(8, 1), 1);
    fbs_params refused = toy(8, 5);
    size_t w = 0;
    CHECK(fbs_pub_key_words(&refused, &w) == FBS_E_INVALID, "k = 5 admitted");
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("public ok\n");
    return 0;
}

/* The client library under AddressSanitizer and UBSan: a stand-alone C program that drives the SOURCES of libfbsclient.so
 * (csrc/fbs_error.cpp, fbs_host.cpp, fbs_client_entries.cpp, fbs_client_capi.cpp, compiled with the sanitizers: make -C tests/c -f client.mk client_asan) through the C
 * ABI of include/fbs_exec.h and nothing else.  Per parameter set -- one k = 1 set and one k = 2 set with two key bits per step --
 * it creates contexts in both seed forms, runs both key generations, exports everything into malloc buffers of EXACTLY the sizes the
 * size entries report (one word more read or written is a sanitizer report), encrypts and decrypts in every form, builds compact and
 * packed words from the header's formulas and decodes them, and walks the refusals.  Prints "<set> ok" per set; exit status 0 only
 * if every check held.  No GPU, no HIP, nothing loaded into an interpreter. */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/fbs_exec.h"

#define Q 0x3FFFFFF84001ull

static int failures = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            printf("FAIL %s:%d: ", __FILE__, __LINE__);    \
            printf(__VA_ARGS__);                           \
            printf("\n");                                  \
            failures++;                                    \
            return 1;                                      \
        }                                                  \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd(void) {   /* splitmix64 */
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static void *xmalloc(size_t bytes) {
    void *p = malloc(bytes ? bytes : 1);
    if (!p) {
        printf("FAIL: out of memory\n");
        exit(2);
    }
    return p;
}

/* field j of `bits` bits into the bit stream of `words` (zeroed by the caller) */
static void put_field(uint64_t *words, size_t j, uint32_t bits, uint64_t v) {
    const size_t b = j * bits, w = b >> 6, o = b & 63;
    words[w] |= v << o;
    if (o + bits > 64) words[w + 1] |= v >> (64 - o);
}

static int refusals(const fbs_params *p) {
    fbs_ctx *ctx = NULL;
    fbs_params bad;
    uint8_t seed32[32] = {1, 2, 3};
    CHECK(fbs_ctx_create(p, 1, 0, &ctx) == FBS_E_DEVICE && !ctx, "device 0 must be refused");
    CHECK(strstr(fbs_last_error(NULL), "libfbsexec") != NULL, "the refusal names the GPU library: %s", fbs_last_error(NULL));
    CHECK(fbs_ctx_create_seeded(p, seed32, 3, &ctx) == FBS_E_DEVICE && !ctx, "device 3 must be refused");
    CHECK(fbs_ctx_create_seeded(p, NULL, FBS_DEVICE_NONE, &ctx) == FBS_E_INVALID, "null seed");
    CHECK(fbs_ctx_create(NULL, 1, FBS_DEVICE_NONE, &ctx) == FBS_E_INVALID && fbs_ctx_create(p, 1, FBS_DEVICE_NONE, NULL) == FBS_E_INVALID, "null arguments");
    CHECK(fbs_poly_size_check(1536) == FBS_E_POLY_SIZE && fbs_poly_size_check(1000) == FBS_E_POLY_SIZE, "non-power-of-two N");
    CHECK(fbs_poly_size_check(8192) == FBS_E_INVALID && fbs_poly_size_check(1024) == FBS_OK, "power-of-two N");
    bad = *p, bad.beta_bsk = 200;   /* would shift by 200 bits were it not refused first */
    CHECK(fbs_ctx_create(&bad, 1, FBS_DEVICE_NONE, &ctx) == FBS_E_INVALID && !ctx, "beta_bsk = 200");
    bad = *p, bad.gamma_ksk = 200;
    CHECK(fbs_ctx_create(&bad, 1, FBS_DEVICE_NONE, &ctx) == FBS_E_INVALID && !ctx, "gamma_ksk = 200");
    bad = *p, bad.log_n_poly = 13;
    CHECK(fbs_ctx_create(&bad, 1, FBS_DEVICE_NONE, &ctx) == FBS_E_INVALID && !ctx, "N = 8192");
    bad = *p, bad.k = 5;
    CHECK(fbs_ctx_create(&bad, 1, FBS_DEVICE_NONE, &ctx) == FBS_E_INVALID && !ctx, "k = 5");
    bad = *p, bad.p_msg = 0;
    CHECK(fbs_ctx_create(&bad, 1, FBS_DEVICE_NONE, &ctx) == FBS_E_INVALID && !ctx, "p = 0");

    CHECK(fbs_ctx_create(p, 1, FBS_DEVICE_NONE, &ctx) == FBS_OK && ctx, "create: %s", fbs_last_error(NULL));
    uint8_t mk[32];
    uint64_t word = 0;
    int64_t msg = 1, stat = -1;
    size_t sizes[2];
    CHECK(fbs_export_seeded_keys(ctx, mk, &word, &word) == FBS_E_STATE, "export before keygen");
    CHECK(fbs_encrypt(ctx, &msg, 1, 0, &word) == FBS_E_STATE && fbs_packing_keygen(ctx, 2, 7) == FBS_E_STATE, "calls before keygen");
    CHECK(fbs_keygen(ctx) == FBS_OK, "keygen");
    CHECK(fbs_export_seeded_keys(ctx, mk, &word, &word) == FBS_E_STATE, "full keys are not seeded keys");
    CHECK(fbs_packing_keygen(ctx, 2, 7) == FBS_E_STATE, "a packing key goes with seeded keys");
    CHECK(fbs_keygen_seeded(ctx) == FBS_OK, "keygen_seeded");
    CHECK(fbs_packing_keygen(ctx, 4, 8) == FBS_E_INVALID && fbs_packing_keygen(ctx, 0, 7) == FBS_E_INVALID &&
              fbs_packing_keygen(ctx, 2, 0) == FBS_E_INVALID && fbs_packing_keygen(ctx, 1, 32) == FBS_E_INVALID, "t_p gamma_p > 31");
    CHECK(fbs_packing_key_sizes(ctx, 0, sizes) == FBS_E_STATE && fbs_export_packing_key(ctx, &word, NULL) == FBS_E_STATE, "no packing key yet");
    CHECK(fbs_encrypt_seeded(ctx, &msg, 1, 1ull << 55, &word) == FBS_E_INVALID && fbs_encrypt(ctx, &msg, 1, 1ull << 55, &word) == FBS_E_INVALID, "explicit nonce at 2^55");
    CHECK(fbs_ctx_stat(ctx, "next_nonce", &stat) == FBS_OK && stat == (int64_t)(1ull << 55), "a refused call moves no counter");
    CHECK(fbs_ctx_stat(ctx, "cu_count", &stat) == FBS_E_INVALID && fbs_ctx_stat(ctx, "scratch_growths", &stat) == FBS_E_INVALID, "device statistics");
    CHECK(fbs_encrypt(ctx, NULL, 1, 0, &word) == FBS_E_INVALID && fbs_decrypt(ctx, &word, 1, NULL) == FBS_E_INVALID, "null buffers");
    CHECK(fbs_encrypt(ctx, NULL, 0, 0, NULL) == FBS_OK, "count 0 does nothing");
    size_t w = 0;
    CHECK(fbs_compact_words(ctx, p->log_n_poly, &w) == FBS_E_INVALID && fbs_compact_words(ctx, 32, &w) == FBS_E_INVALID, "compact widths");
    CHECK(fbs_packed_words(ctx, 5, 32, &w) == FBS_E_INVALID && fbs_packed_words(ctx, (size_t)-1, 31, &w) == FBS_E_INVALID, "packed widths and counts");
    static const int want[5] = {FBS_E_NOMEM, FBS_E_NOMEM, FBS_E_INVALID, FBS_E_INVALID, FBS_OK};
    for (int kind = 0; kind < 5; kind++) {
        CHECK(fbs_debug_raise(ctx, kind) == want[kind] && fbs_debug_raise(NULL, kind) == want[kind], "fbs_debug_raise(%d)", kind);
        if (want[kind]) CHECK(fbs_last_error(ctx)[0] && fbs_last_error(NULL)[0], "no text for kind %d", kind);
    }
    CHECK(strcmp(fbs_device_info(ctx), "host") == 0, "device info: %s", fbs_device_info(ctx));
    fbs_ctx_destroy(ctx);
    fbs_ctx_destroy(NULL);
    return 0;
}

static int run_set(const char *name, const fbs_params *p) {
    const uint32_t N = 1u << p->log_n_poly, n = p->n, k = p->k, D = k * N;
    const uint64_t two_p = 2ull * p->p_msg, delta = 2 * ((Q + 2ull * p->p_msg) / (4ull * p->p_msg));
    const size_t count = 3 * two_p;
    if (refusals(p)) return 1;

    for (int form = 0; form < 2; form++) {   /* 0: 64-bit seed, 1: 32 bytes */
        fbs_ctx *ctx = NULL, *twin = NULL;
        uint8_t seed32[32];
        for (int i = 0; i < 32; i++) seed32[i] = (uint8_t)(7 * i + 1);
        if (form == 0) {
            CHECK(fbs_ctx_create(p, 11, FBS_DEVICE_NONE, &ctx) == FBS_OK && fbs_ctx_create(p, 11, FBS_DEVICE_NONE, &twin) == FBS_OK, "create: %s", fbs_last_error(NULL));
        } else {
            CHECK(fbs_ctx_create_seeded(p, seed32, FBS_DEVICE_NONE, &ctx) == FBS_OK && fbs_ctx_create_seeded(p, seed32, FBS_DEVICE_NONE, &twin) == FBS_OK, "create: %s", fbs_last_error(NULL));
        }
        int64_t stat = 0;
        CHECK(fbs_ctx_stat(ctx, "has_secret", &stat) == FBS_OK && stat == 0, "has_secret before keygen");

        /* full keys into exactly-sized buffers; the twin makes the same words */
        size_t ks[4];
        CHECK(fbs_key_sizes(ctx, ks) == FBS_OK && ks[0] == n && ks[1] == D, "key sizes");
        CHECK(fbs_keygen(ctx) == FBS_OK && fbs_keygen(twin) == FBS_OK, "keygen: %s", fbs_last_error(ctx));
        uint64_t *key[4], *key2[4];
        for (int i = 0; i < 4; i++) key[i] = xmalloc(ks[i] * 8), key2[i] = xmalloc(ks[i] * 8);
        CHECK(fbs_export_keys(ctx, key[0], key[1], key[2], key[3]) == FBS_OK, "export_keys: %s", fbs_last_error(ctx));
        CHECK(fbs_export_keys(twin, key2[0], key2[1], key2[2], key2[3]) == FBS_OK, "export_keys (twin)");
        for (int i = 0; i < 4; i++) CHECK(memcmp(key[i], key2[i], ks[i] * 8) == 0, "%s: key %d differs between two contexts of one seed", name, i);
        for (size_t i = 0; i < ks[0]; i++) CHECK(key[0][i] <= 1, "sk_lwe is binary");
        for (size_t i = 0; i < ks[2]; i++) CHECK(key[2][i] < Q, "bsk word %zu is not canonical", i);
        CHECK(fbs_export_keys(ctx, NULL, NULL, NULL, key[3]) == FBS_OK, "export_keys with null pointers");

        /* encrypt / decrypt, explicit and fresh streams */
        int64_t *msgs = xmalloc(count * 8), *back = xmalloc(count * 8);
        for (size_t i = 0; i < count; i++) msgs[i] = (int64_t)(i % two_p);
        uint64_t *cts = xmalloc(count * (D + 1) * 8), *cts2 = xmalloc(count * (D + 1) * 8);
        CHECK(fbs_encrypt(ctx, msgs, count, 5, cts) == FBS_OK && fbs_encrypt(twin, msgs, count, 5, cts2) == FBS_OK, "encrypt: %s", fbs_last_error(ctx));
        CHECK(memcmp(cts, cts2, count * (D + 1) * 8) == 0, "encrypt is not reproducible");
        CHECK(fbs_decrypt(ctx, cts, count, back) == FBS_OK && memcmp(msgs, back, count * 8) == 0, "decrypt");
        uint64_t first = 0, second = 0;
        CHECK(fbs_encrypt_fresh(ctx, msgs, count, cts, &first) == FBS_OK && first == 1ull << 55, "first fresh stream %" PRIu64, first);
        CHECK(fbs_encrypt_fresh(ctx, msgs, count, cts2, &second) == FBS_OK && second == first + count, "second fresh stream");
        CHECK(memcmp(cts, cts2, count * (D + 1) * 8) != 0, "two fresh calls share streams");
        CHECK(fbs_decrypt(ctx, cts2, count, back) == FBS_OK && memcmp(msgs, back, count * 8) == 0, "decrypt of fresh ciphertexts");
        CHECK(fbs_encrypt_fresh(ctx, msgs, 1, cts, NULL) == FBS_OK, "fresh with a null nonce pointer");

        /* seeded keys: bodies into exactly-sized buffers; the secrets are fbs_keygen's */
        size_t ss[2];
        CHECK(fbs_keygen_seeded(ctx) == FBS_OK && fbs_seeded_key_sizes(ctx, ss) == FBS_OK, "keygen_seeded: %s", fbs_last_error(ctx));
        CHECK(ss[0] * (k + 1) == ks[2] && ss[1] * (n + 1) == ks[3], "seeded sizes");
        uint8_t mk[32];
        uint64_t *bb = xmalloc(ss[0] * 8), *kb = xmalloc(ss[1] * 8);
        CHECK(fbs_export_seeded_keys(ctx, mk, bb, kb) == FBS_OK, "export_seeded_keys: %s", fbs_last_error(ctx));
        CHECK(fbs_export_keys(ctx, key2[0], key2[1], key2[2], key2[3]) == FBS_OK, "export_keys after keygen_seeded");
        CHECK(memcmp(key[0], key2[0], ks[0] * 8) == 0 && memcmp(key[1], key2[1], ks[1] * 8) == 0, "seeded secrets differ from fbs_keygen's");
        for (size_t r = 0; r < ss[1]; r++) CHECK(kb[r] == key2[3][r * (n + 1) + n], "ksk body %zu", r);
        for (size_t r = 0; r < ss[0] / N; r++) CHECK(memcmp(bb + r * N, key2[2] + (r * (k + 1) + k) * (size_t)N, N * 8) == 0, "bsk body row %zu", r);
        CHECK(fbs_ctx_stat(ctx, "seeded_keys", &stat) == FBS_OK && stat == 1, "seeded_keys");

        /* seeded inputs: encrypt, expand, decrypt */
        uint64_t *bodies = xmalloc(count * 8);
        CHECK(fbs_encrypt_seeded(ctx, msgs, count, 9, bodies) == FBS_OK, "encrypt_seeded: %s", fbs_last_error(ctx));
        CHECK(fbs_expand_seeded(ctx, bodies, count, 9, cts) == FBS_OK, "expand_seeded: %s", fbs_last_error(ctx));
        for (size_t i = 0; i < count; i++) CHECK(cts[i * (D + 1) + D] == bodies[i], "body %zu", i);
        CHECK(fbs_decrypt(ctx, cts, count, back) == FBS_OK && memcmp(msgs, back, count * 8) == 0, "seeded round trip");
        CHECK(fbs_encrypt_seeded_fresh(ctx, msgs, count, bodies, &first) == FBS_OK && first == second + count + 1, "seeded fresh stream %" PRIu64, first);
        CHECK(fbs_expand_seeded(ctx, bodies, count, first, cts) == FBS_OK && fbs_decrypt(ctx, cts, count, back) == FBS_OK &&
                  memcmp(msgs, back, count * 8) == 0, "seeded fresh round trip");

        /* compact outputs: small-key ciphertexts under the exported sk_lwe, rounded and packed by the header's formulas */
        for (int wi = 0; wi < 2; wi++) {
            const uint32_t bits = wi ? 31 : p->log_n_poly + 1, sh = 46 - bits;
            size_t W = 0;
            CHECK(fbs_compact_words(ctx, bits, &W) == FBS_OK && W == ((size_t)(n + 1) * bits + 63) / 64, "compact_words");
            uint64_t *words = xmalloc(count * W * 8);
            memset(words, 0, count * W * 8);
            for (size_t c = 0; c < count; c++) {
                uint64_t body = ((uint64_t)msgs[c] * delta + rnd() % 64) % Q;
                int64_t eps = 0;
                for (uint32_t i = 0; i < n; i++) {
                    const uint64_t x = rnd() % Q, m = ((x >> (sh - 1)) + 1) >> 1;
                    if (key[0][i]) body = (body + x) % Q;
                    eps += (int64_t)x - (int64_t)(m << sh);
                    put_field(words + c * W, i, bits, m & ((1ull << bits) - 1));
                }
                const int64_t half = eps >= 0 ? eps / 2 : -((-eps + 1) / 2);   /* floor(eps / 2) */
                body = (uint64_t)(((int64_t)body - half) % (int64_t)Q + (int64_t)Q) % Q;
                put_field(words + c * W, n, bits, (((body >> (sh - 1)) + 1) >> 1) & ((1ull << bits) - 1));
            }
            CHECK(fbs_decrypt_compact(ctx, words, count, bits, back) == FBS_OK, "decrypt_compact: %s", fbs_last_error(ctx));
            CHECK(memcmp(msgs, back, count * 8) == 0, "%s: compact messages at %u bits", name, bits);
            free(words);
        }

        /* packing key, then packed outputs: one full GLWE sample and a partly filled one under the exported sk_glwe */
        CHECK(fbs_packing_keygen(ctx, 2, 7) == FBS_OK, "packing_keygen: %s", fbs_last_error(ctx));
        size_t ps[2];
        CHECK(fbs_packing_key_sizes(ctx, 0, ps) == FBS_OK && ps[0] == (size_t)n * 2 * N && ps[1] == ps[0] * (k + 1), "packing sizes");
        uint64_t *pb = xmalloc(ps[0] * 8), *pf = xmalloc(ps[1] * 8);
        CHECK(fbs_export_packing_key(ctx, pb, pf) == FBS_OK, "export_packing_key");
        for (size_t r = 0; r < (size_t)n * 2; r++) CHECK(memcmp(pb + r * N, pf + (r * (k + 1) + k) * (size_t)N, N * 8) == 0, "packing row %zu", r);
        CHECK(fbs_ctx_stat(ctx, "packing_levels", &stat) == FBS_OK && stat == 2 && fbs_ctx_stat(ctx, "packing_base_bits", &stat) == FBS_OK && stat == 7, "packing statistics");
        {
            const uint32_t bits = 20, fill2 = 37;
            const size_t pcount = N + fill2;
            size_t PW = 0;
            CHECK(fbs_packed_words(ctx, pcount, bits, &PW) == FBS_OK, "packed_words");
            const size_t full_words = (size_t)(k + 1) * N * bits / 64;
            CHECK(PW == full_words + (size_t)k * N * bits / 64 + ((size_t)fill2 * bits + 63) / 64, "packed_words = %zu", PW);
            uint64_t *words = xmalloc(PW * 8), *a = xmalloc((size_t)D * 8), *b = xmalloc((size_t)N * 8);
            int64_t *pm = xmalloc(pcount * 8), *pback = xmalloc(pcount * 8);
            memset(words, 0, PW * 8);
            for (size_t i = 0; i < pcount; i++) pm[i] = (int64_t)(rnd() % two_p);
            for (size_t g = 0; g * N < pcount; g++) {
                const uint32_t fill = g ? fill2 : N;
                uint64_t *sample = words + g * full_words;
                for (uint32_t j = 0; j < N; j++) b[j] = ((j < fill ? (uint64_t)pm[g * N + j] * delta : 0) + rnd() % 8) % Q;
                for (uint32_t c = 0; c < k; c++)
                    for (uint32_t i = 0; i < N; i++) {
                        const uint64_t x = a[c * N + i] = rnd() % Q;
                        for (uint32_t s = 0; s < N; s++) {   /* b += x X^i S_c (negacyclic) */
                            if (!key[1][c * N + s]) continue;
                            const uint32_t j = i + s;
                            if (j < N) b[j] = (b[j] + x) % Q;
                            else b[j - N] = (b[j - N] + Q - x) % Q;
                        }
                    }
                for (uint32_t f = 0; f < D; f++) put_field(sample, f, bits, (((a[f] >> (45 - bits)) + 1) >> 1) & ((1ull << bits) - 1));
                for (uint32_t j = 0; j < fill; j++) put_field(sample, D + j, bits, (((b[j] >> (45 - bits)) + 1) >> 1) & ((1ull << bits) - 1));
            }
            CHECK(fbs_decrypt_packed(ctx, words, pcount, bits, pback) == FBS_OK, "decrypt_packed: %s", fbs_last_error(ctx));
            CHECK(memcmp(pm, pback, pcount * 8) == 0, "%s: packed messages", name);
            free(words), free(a), free(b), free(pm), free(pback);
        }

        free(pb), free(pf), free(bodies), free(bb), free(kb), free(cts), free(cts2), free(msgs), free(back);
        for (int i = 0; i < 4; i++) free(key[i]), free(key2[i]);
        fbs_ctx_destroy(ctx);
        fbs_ctx_destroy(twin);
    }
    printf("%s ok\n", name);
    return 0;
}

int main(void) {
    const fbs_params k1 = {.n = 10, .log_n_poly = 8, .k = 1, .l_bsk = 2, .beta_bsk = 10, .t_ksk = 8, .gamma_ksk = 2, .p_msg = 7,
                           .sigma_lwe = 1 << 8, .sigma_glwe = 1 << 4, .bsk_group = 1, .reserved = 0};
    const fbs_params k2 = {.n = 10, .log_n_poly = 8, .k = 2, .l_bsk = 1, .beta_bsk = 21, .t_ksk = 8, .gamma_ksk = 2, .p_msg = 7,
                           .sigma_lwe = 1 << 8, .sigma_glwe = 4, .bsk_group = 2, .reserved = 0};
    run_set("k=1 N=256 group=1", &k1);
    run_set("k=2 N=256 group=2", &k2);
    if (failures) printf("%d check(s) failed\n", failures);
    return failures ? 1 : 0;
}

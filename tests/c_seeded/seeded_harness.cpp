// Sanitizer harness for the host side of the seeded path (csrc/fbs_host.cpp: host_keygen_seeded, host_expand_seeded_keys,
// host_encrypt_seeded, host_expand_seeded).  Built by tests/test_seeded_abi.py with g++ -fsanitize=address,undefined from the
// sources and flags tests/c/Makefile builds host_harness from (fbs_plan.cpp, fbs_host.cpp, fbs_select.cpp); no GPU, no HIP call.
// At toy parameter sets (k = 1, 2, 3; bsk_group 1 and 2; l = 1 and 2) it checks, and prints "<set> ok" per set:
//   * every row of the seeded keys has the phase the fbs_key_sizes layout says it encrypts, plus exactly the noise sample of
//     its seeded noise stream;
//   * expanding (mask key, bodies) reproduces the generated keys word for word;
//   * the noise of every seeded row differs from that of the matching fbs_keygen row (stream separation);
//   * the mask key is the first 32 bytes of block 0 of stream (DOM_MASK_KEY, 0), and changing one of its bytes changes every
//     expanded mask;
//   * seeded ciphertexts expand and decrypt to their messages, with the noise of their stream.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../tfhe_fbs_map_amd/csrc/fbs_chacha.hpp"
#include "../../tfhe_fbs_map_amd/csrc/fbs_internal.hpp"

namespace fbs {
int set_error(const fbs_ctx *ctx, int code, const std::string &msg) {   // (the product's lives in fbs_capi.cpp, beside the HIP calls)
    if (ctx) ctx->err = msg;
    return code;
}
}  // namespace fbs
using namespace fbs;

static int failures = 0;
#define CHECK(cond, ...)                          \
    do {                                          \
        if (!(cond)) {                            \
            printf("FAIL %s:%d ", __FILE__, __LINE__); \
            printf(__VA_ARGS__);                  \
            printf("\n");                         \
            failures++;                           \
            return 1;                             \
        }                                         \
    } while (0)

// the residual of every key row: phase minus the message the layout names (row order of fbs_key_sizes)
static void bsk_residuals(const fbs_ctx &c, const std::vector<uint64_t> &bsk, std::vector<uint64_t> &res) {
    const uint32_t N = c.N, k = c.p.k, l = c.p.l_bsk, rows = c.rows;
    res.assign(c.n_ggsw * rows * N, 0);
    for (size_t r = 0; r < c.n_ggsw * rows; r++) {
        const size_t g = r / rows;
        const uint32_t rr = (uint32_t)(r % rows), comp = rr / l, lv = rr % l;
        uint64_t bit = c.group == 2 ? 0 : c.sk_lwe[g];
        if (c.group == 2) {
            const uint64_t s0 = c.sk_lwe[2 * (g / 3)], s1 = c.sk_lwe[2 * (g / 3) + 1];
            bit = g % 3 == 0 ? (s0 & (1 - s1)) : g % 3 == 1 ? ((1 - s0) & s1) : (s0 & s1);
        }
        const uint64_t *row = bsk.data() + r * (size_t)(k + 1) * N;
        uint64_t *ph = res.data() + r * N;
        for (uint32_t j = 0; j < N; j++) ph[j] = row[(size_t)k * N + j];
        for (uint32_t cc = 0; cc < k; cc++)
            for (uint32_t sh = 0; sh < N; sh++) {
                if (!c.sk_glwe[(size_t)cc * N + sh]) continue;
                for (uint32_t j = 0; j < N; j++) {
                    const uint64_t a = row[(size_t)cc * N + j];
                    if (j + sh < N) ph[j + sh] = fq_sub(ph[j + sh], a);
                    else ph[j + sh - N] = fq_add(ph[j + sh - N], a);
                }
            }
        for (uint32_t j = 0; j < N; j++) {
            uint64_t want = 0;
            if (bit && comp == k && j == 0) want = c.g[lv];
            if (bit && comp < k && c.sk_glwe[(size_t)comp * N + j]) want = fq_sub(0, c.g[lv]);
            ph[j] = fq_sub(ph[j], want);
        }
    }
}

static void ksk_residuals(const fbs_ctx &c, const std::vector<uint64_t> &ksk, std::vector<uint64_t> &res) {
    const uint32_t n = c.p.n, t = c.p.t_ksk;
    res.assign((size_t)c.D * t, 0);
    for (size_t r = 0; r < res.size(); r++) {
        const uint32_t j = (uint32_t)(r / t), v = (uint32_t)(r % t);
        const uint64_t *row = ksk.data() + r * (n + 1);
        uint64_t ph = row[n];
        for (uint32_t i = 0; i < n; i++)
            if (c.sk_lwe[i]) ph = fq_sub(ph, row[i]);
        res[r] = fq_sub(ph, c.sk_glwe[j] ? c.h[v] : 0);
    }
}

struct Set {
    uint32_t n, log_n, k, l, beta, t, gamma, p, group;
};

static int run_set(const Set &s) {
    fbs_params p{};
    p.n = s.n, p.log_n_poly = s.log_n, p.k = s.k, p.l_bsk = s.l, p.beta_bsk = s.beta, p.t_ksk = s.t, p.gamma_ksk = s.gamma, p.p_msg = s.p;
    p.sigma_lwe = 1ull << 30, p.sigma_glwe = 1ull << 30, p.bsk_group = s.group;   // wide noise: no two rows' noise meet by chance
    fbs_ctx full, seeded;
    CHECK(host_ctx_init(&full, &p, 7, nullptr) == FBS_OK && host_ctx_init(&seeded, &p, 7, nullptr) == FBS_OK, "host_ctx_init: %s", full.err.c_str());
    host_keygen(&full);
    host_keygen_seeded(&seeded);
    const uint32_t N = seeded.N, D = seeded.D, n = p.n, k = p.k, t = p.t_ksk;
    const size_t bsk_rows = seeded.n_ggsw * seeded.rows, ksk_rows = (size_t)D * t;
    CHECK(seeded.sk_lwe == full.sk_lwe && seeded.sk_glwe == full.sk_glwe, "secrets differ from fbs_keygen's");
    CHECK(seeded.bsk.size() == full.bsk.size() && seeded.ksk.size() == full.ksk.size(), "key sizes");

    // the mask key: the first four words of block 0 of stream (DOM_MASK_KEY, 0) under the context's key
    uint64_t blk[8];
    chacha_block(seeded.rkey.w, (uint64_t)DOM_MASK_KEY << 56, 0, blk);
    for (int i = 0; i < 4; i++)
        CHECK(seeded.mask_key.w[2 * i] == (uint32_t)blk[i] && seeded.mask_key.w[2 * i + 1] == (uint32_t)(blk[i] >> 32), "mask key word %d", i);

    // phases: the layout's message plus exactly the seeded noise sample; fbs_keygen's rows carry their own streams' noise
    std::vector<uint64_t> rs, rf;
    bsk_residuals(seeded, seeded.bsk, rs);
    bsk_residuals(full, full.bsk, rf);
    for (size_t r = 0; r < bsk_rows; r++) {
        for (uint32_t j = 0; j < N; j++) {
            CHECK(rs[r * N + j] == fq_from_i64(noise_sample(seeded.rkey, stream_id(DOM_SBSK_NOISE, r), j, p.sigma_glwe)), "bsk row %zu coefficient %u", r, j);
            CHECK(rf[r * N + j] == fq_from_i64(noise_sample(full.rkey, stream_id(DOM_BSK_NOISE, r), j, p.sigma_glwe)), "fbs_keygen bsk row %zu", r);
        }
        CHECK(std::memcmp(&rs[r * N], &rf[r * N], N * 8) != 0, "bsk row %zu: seeded noise equals fbs_keygen's", r);
    }
    ksk_residuals(seeded, seeded.ksk, rs);
    ksk_residuals(full, full.ksk, rf);
    for (size_t r = 0; r < ksk_rows; r++) {
        CHECK(rs[r] == fq_from_i64(noise_sample(seeded.rkey, stream_id(DOM_SKSK_NOISE, r), 0, p.sigma_lwe)), "ksk row %zu", r);
        CHECK(rs[r] != rf[r], "ksk row %zu: seeded noise equals fbs_keygen's", r);
    }

    // bodies -> full keys, word for word
    std::vector<uint64_t> bb(bsk_rows * N), kb(ksk_rows);
    for (size_t r = 0; r < bsk_rows; r++) std::memcpy(&bb[r * N], &seeded.bsk[(r * (k + 1) + k) * (size_t)N], N * 8);
    for (size_t r = 0; r < ksk_rows; r++) kb[r] = seeded.ksk[r * (n + 1) + n];
    std::vector<uint64_t> bsk2, ksk2;
    host_expand_seeded_keys(&seeded, seeded.mask_key, bb.data(), kb.data(), bsk2, ksk2);
    CHECK(bsk2 == seeded.bsk && ksk2 == seeded.ksk, "expanded keys differ from the generated ones");
    for (size_t i = 0; i < seeded.bsk.size(); i++) CHECK(seeded.bsk[i] < FQ, "bsk word %zu not canonical", i);

    // one byte of the mask key changed: every mask row changes, the bodies stay
    RandKey other = seeded.mask_key;
    other.w[5] ^= 0x100u;
    host_expand_seeded_keys(&seeded, other, bb.data(), kb.data(), bsk2, ksk2);
    for (size_t r = 0; r < bsk_rows; r++) {
        const size_t base = r * (size_t)(k + 1) * N;
        CHECK(std::memcmp(&bsk2[base], &seeded.bsk[base], (size_t)k * N * 8) != 0, "bsk mask row %zu unchanged", r);
        CHECK(std::memcmp(&bsk2[base + (size_t)k * N], &seeded.bsk[base + (size_t)k * N], (size_t)N * 8) == 0, "bsk body %zu", r);
    }
    for (size_t r = 0; r < ksk_rows; r++)
        CHECK(std::memcmp(&ksk2[r * (n + 1)], &seeded.ksk[r * (n + 1)], (size_t)n * 8) != 0, "ksk mask row %zu unchanged", r);

    // seeded ciphertexts: bodies -> full ciphertexts that decrypt to the messages, with their stream's noise
    const size_t count = 37;
    const uint64_t nonce0 = (1ull << 55) - 40;
    std::vector<int64_t> msgs(count), back(count);
    for (size_t i = 0; i < count; i++) msgs[i] = (int64_t)((i * 5 + 3) % (2 * p.p_msg));
    std::vector<uint64_t> bodies(count), cts(count * (D + 1)), cts2(count * (D + 1));
    host_encrypt_seeded(&seeded, msgs.data(), count, nonce0, bodies.data());
    host_expand_seeded(&seeded, bodies.data(), count, nonce0, cts.data());
    host_decrypt(&seeded, cts.data(), count, back.data());
    CHECK(back == msgs, "seeded ciphertexts do not decrypt to their messages");
    for (size_t i = 0; i < count; i++) {
        const uint64_t *ct = &cts[i * (D + 1)];
        uint64_t ph = ct[D];
        for (uint32_t j = 0; j < D; j++)
            if (seeded.sk_glwe[j]) ph = fq_sub(ph, ct[j]);
        const uint64_t want = fq_add(fq_mul(fq_from_i64(msgs[i]), 2 * seeded.delta_half),
                                     fq_from_i64(noise_sample(seeded.rkey, stream_id(DOM_SENC_NOISE, nonce0 + i), 0, p.sigma_glwe)));
        CHECK(ph == want, "seeded ciphertext %zu: phase", i);
    }
    const RandKey mine = seeded.mask_key;
    seeded.mask_key = other;
    host_expand_seeded(&seeded, bodies.data(), count, nonce0, cts2.data());
    seeded.mask_key = mine;
    for (size_t i = 0; i < count; i++)
        CHECK(std::memcmp(&cts2[i * (D + 1)], &cts[i * (D + 1)], (size_t)D * 8) != 0, "ciphertext mask %zu unchanged", i);
    // full encryption on the same context keeps working (the secrets are fbs_keygen's)
    host_encrypt(&seeded, msgs.data(), count, 5, cts2.data());
    host_decrypt(&seeded, cts2.data(), count, back.data());
    CHECK(back == msgs, "full encryption on a seeded context");
    return 0;
}

int main() {
    const Set sets[] = {{12, 8, 1, 2, 9, 8, 2, 7, 1}, {12, 8, 1, 1, 20, 6, 3, 7, 2}, {8, 8, 2, 1, 21, 8, 2, 7, 2},
                        {10, 8, 2, 2, 10, 5, 3, 15, 1}, {8, 8, 3, 1, 18, 4, 4, 7, 2}, {6, 8, 3, 2, 9, 3, 5, 7, 1}};
    for (const Set &s : sets) {
        if (run_set(s)) continue;
        printf("k=%u l=%u group=%u ok\n", s.k, s.l, s.group);
    }
    return failures ? 1 : 0;
}

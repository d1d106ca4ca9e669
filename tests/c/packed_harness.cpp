// Sanitizer harness for the HOST side of packed outputs (include/fbs_exec.h, "packed outputs"): csrc/fbs_host.cpp's
// host_gadget_keygen, host_expand_gadget_key (GK_PACK) and host_decrypt_packed with the arithmetic of csrc/fbs_pack.hpp, built by
// tests/test_packed_abi.py with g++ and the -fsanitize=address,undefined flags of tests/c/Makefile.  No GPU, no HIP call.
//
//   packed_harness keys      at two toy sets and several (t_p, gamma_p): the key a client generates and the key a server expands from
//                            (mask key, bodies) are identical; every row's phase minus s_i h_v is within 6 sigma_glwe; the digits of
//                            pack_digit recompose to the rounded field; out-of-range (t_p, gamma_p) are refused.  "ok keys ..." lines.
//   packed_harness decode    noiseless packed samples built from the secret at every width, full and partial fill, in buffers of
//                            exactly packed_words words: host_decrypt_packed returns the messages.  "ok decode ..." lines.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../tfhe_fbs_map_amd/csrc/fbs_internal.hpp"
#include "../../tfhe_fbs_map_amd/csrc/fbs_pack.hpp"

using namespace fbs;

static bool make_ctx(fbs_ctx &ctx, uint32_t n, uint32_t log_n, uint32_t k, uint32_t p, uint64_t seed) {
    fbs_params prm{};
    prm.n = n, prm.log_n_poly = log_n, prm.k = k, prm.l_bsk = 1, prm.beta_bsk = 18, prm.t_ksk = 4, prm.gamma_ksk = 3, prm.p_msg = p;
    prm.sigma_lwe = 1 << 8, prm.sigma_glwe = 1 << 4, prm.bsk_group = 1;
    if (host_ctx_init(&ctx, &prm, seed, nullptr) != FBS_OK) {
        printf("FAIL host_ctx_init: %s\n", ctx.err.c_str());
        return false;
    }
    host_keygen_seeded(&ctx);   // the secrets, the mask key (and the other seeded keys: toy sizes)
    return true;
}

static int mode_keys() {
    int failures = 0;
    const uint32_t shapes[2][3] = {{6, 8, 1}, {4, 8, 2}};   // (n, log N, k)
    const uint32_t keys[4][2] = {{1, 8}, {2, 7}, {3, 10}, {1, 31}};
    for (auto &sh : shapes)
        for (auto &tk : keys) {
            const uint32_t n = sh[0], k = sh[2], t = tk[0], gamma = tk[1];
            fbs_ctx ctx;
            if (!make_ctx(ctx, n, sh[1], k, 7, 5)) return 1;
            const uint32_t N = ctx.N;
            if (gadget_params_refused(t, gamma)) {
                printf("FAIL (%u, %u) refused\n", t, gamma);
                return 1;
            }
            std::vector<uint64_t> bodies, client, server;
            host_gadget_keygen(&ctx, GK_PACK, t, gamma, bodies);
            host_expand_gadget_key(&ctx, GK_PACK, ctx.mask_key, t, bodies.data(), client);
            // the server: another context of the same set, no secret, the client's mask key
            fbs_ctx srv;
            if (!make_ctx(srv, n, sh[1], k, 7, 99)) return 1;
            srv.sk_lwe.clear(), srv.sk_glwe.clear();
            host_expand_gadget_key(&srv, GK_PACK, ctx.mask_key, t, bodies.data(), server);
            if (client != server || client.size() != (size_t)n * t * (k + 1) * N) {
                printf("FAIL client and server keys differ n=%u k=%u t=%u\n", n, k, t);
                failures++;
            }
            int64_t worst = 0;
            for (uint32_t i = 0; i < n; i++)
                for (uint32_t v = 0; v < t; v++) {
                    const uint64_t *row = client.data() + ((size_t)i * t + v) * (k + 1) * N;
                    std::vector<uint64_t> phase(row + (size_t)k * N, row + (size_t)(k + 1) * N);
                    for (uint32_t c = 0; c < k; c++)
                        for (uint32_t s = 0; s < N; s++) {
                            if (!ctx.sk_glwe[(size_t)c * N + s]) continue;
                            const uint64_t *a = row + (size_t)c * N;
                            for (uint32_t j = 0; j < N - s; j++) phase[j + s] = fq_sub(phase[j + s], a[j]);
                            for (uint32_t j = N - s; j < N; j++) phase[j + s - N] = fq_add(phase[j + s - N], a[j]);
                        }
                    if (ctx.sk_lwe[i]) phase[0] = fq_sub(phase[0], pack_gadget(gamma, v));
                    for (uint32_t j = 0; j < N; j++) {
                        const int64_t e = phase[j] > FQ / 2 ? -(int64_t)(FQ - phase[j]) : (int64_t)phase[j];
                        worst = std::max<int64_t>(worst, e < 0 ? -e : e);
                    }
                }
            if (worst == 0 || worst > 6 * (int64_t)ctx.p.sigma_glwe) {
                printf("FAIL row phase %lld beyond 6 sigma n=%u k=%u t=%u gamma=%u\n", (long long)worst, n, k, t, gamma);
                failures++;
            }
            // digits: balanced, and sum_v d_v 2^(gamma (t-1-v)) = a' mod 2^(t gamma)
            std::mt19937_64 rng(t * 100 + gamma);
            const uint32_t tg = t * gamma, offs = pack_digit_offsets(t, gamma);
            for (int it = 0; it < 2000; it++) {
                static const uint32_t edge[4] = {0u, 0x7fffffffu, 0x40000000u, 0x3fffffffu};
                const uint32_t m = it < 4 ? edge[it] : (uint32_t)rng() & 0x7fffffffu;
                const uint32_t a = pack_round_mask(m, tg), z = (uint32_t)(((uint64_t)a + offs) & ((1ull << tg) - 1));
                int64_t sum = 0;
                for (uint32_t v = 0; v < t; v++) {
                    const int64_t d = pack_digit(z, v, t, gamma);
                    if (d < -(1ll << (gamma - 1)) || d >= (1ll << (gamma - 1))) failures++, printf("FAIL digit range\n");
                    sum += d * (1ll << (gamma * (t - 1 - v)));
                }
                if (((sum - (int64_t)a) & ((1ll << tg) - 1)) != 0 || a >= (1ull << tg)) failures++, printf("FAIL digits of %u\n", m);
                if (pack_lift_body(m) != (uint64_t)(((unsigned __int128)m * FQ + (1u << 30)) >> 31) || pack_lift_body(m) >= FQ)
                    failures++, printf("FAIL lift of %u\n", m);
            }
            printf("ok keys n=%u k=%u t=%u gamma=%u worst=%lld\n", n, k, t, gamma, (long long)worst);
        }
    const uint32_t bad[][2] = {{0, 5}, {5, 0}, {4, 8}, {2, 16}, {1, 32}, {32, 1}, {0xFFFFFFFFu, 0xFFFFFFFFu}, {65536, 65536}, {0x80000000u, 2}};
    for (auto &b : bad)
        if (!gadget_params_refused(b[0], b[1])) {
            printf("FAIL (%u, %u) accepted\n", b[0], b[1]);
            failures++;
        }
    printf("ok keys refusals\n");
    return failures ? 1 : 0;
}

static int mode_decode() {
    std::mt19937_64 rng(777);
    int failures = 0;
    const uint32_t shapes[2][3] = {{6, 8, 1}, {4, 8, 2}};
    for (auto &sh : shapes) {
        const uint32_t k = sh[2], p = sh[2] == 1 ? 7 : 15;
        fbs_ctx ctx;
        if (!make_ctx(ctx, sh[0], sh[1], k, p, 8)) return 1;
        const uint32_t N = ctx.N;
        for (uint32_t bits = sh[1] + 1; bits <= 31; bits++) {
            const uint32_t mask = (uint32_t)((1ull << bits) - 1);
            for (size_t count : {(size_t)1, (size_t)N - 1, (size_t)N, (size_t)N + 1, (size_t)2 * N + 3}) {
                std::vector<uint64_t> words(packed_words(k, N, count, bits));   // exactly: a read past the batch is a finding
                std::vector<int64_t> msgs(count), back(count, -1);
                size_t w0 = 0;
                for (size_t g = 0; g * N < count; g++) {
                    const uint32_t fill = (uint32_t)std::min<size_t>(N, count - g * N);
                    std::vector<uint32_t> f((size_t)k * N + fill), sum(N, 0);
                    for (uint32_t c = 0; c < k; c++)
                        for (uint32_t j = 0; j < N; j++) f[(size_t)c * N + j] = (uint32_t)rng() & mask;
                    for (uint32_t c = 0; c < k; c++)
                        for (uint32_t s = 0; s < N; s++) {
                            if (!ctx.sk_glwe[(size_t)c * N + s]) continue;
                            for (uint32_t j = 0; j < N - s; j++) sum[j + s] += f[(size_t)c * N + j];
                            for (uint32_t j = N - s; j < N; j++) sum[j + s - N] -= f[(size_t)c * N + j];
                        }
                    for (uint32_t j = 0; j < fill; j++) {
                        msgs[g * N + j] = (int64_t)(rng() % (2 * p));
                        const uint64_t centre = (((uint64_t)msgs[g * N + j] << bits) + p) / (2 * p);
                        f[(size_t)k * N + j] = (uint32_t)(sum[j] + centre) & mask;
                    }
                    const size_t W = packed_sample_words(k, N, fill, bits);
                    for (size_t j = 0; j < W; j++)
                        words[w0 + j] = compact_word((uint32_t)j, (uint32_t)f.size(), bits, [&](uint32_t i) { return f[i]; });
                    w0 += W;
                }
                if (w0 != words.size()) failures++, printf("FAIL packed_words k=%u bits=%u count=%zu\n", k, bits, count);
                host_decrypt_packed(&ctx, words.data(), count, bits, back.data());
                if (back != msgs) failures++, printf("FAIL decode k=%u bits=%u count=%zu\n", k, bits, count);
            }
            printf("ok decode k=%u bits=%u\n", k, bits);
        }
        host_decrypt_packed(&ctx, nullptr, 0, 12, nullptr);   // count = 0 touches nothing
    }
    return failures ? 1 : 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && !strcmp(argv[1], "keys")) return mode_keys();
    if (argc >= 2 && !strcmp(argv[1], "decode")) return mode_decode();
    fprintf(stderr, "usage: packed_harness keys | decode\n");
    return 2;
}

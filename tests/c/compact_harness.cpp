// Sanitizer harness for the HOST decode of compact output ciphertexts (include/fbs_exec.h, "compact outputs"):
// csrc/fbs_host.cpp's host_decrypt_compact and host_compact_trivial with the arithmetic of csrc/fbs_compact.hpp, built by
// tests/test_compact_abi.py with g++ and the -fsanitize=address,undefined flags of tests/c/Makefile.  No GPU, no HIP call.
//
//   compact_harness roundtrip     compact ciphertexts made in the clear under random small keys, at every width and several n:
//                                 packed into buffers of exactly count * W words (so that a read past a ciphertext is a finding),
//                                 decoded, checked; the compaction of trivial ciphertexts against host_decrypt of the trivial
//                                 ciphertext itself.  Prints "ok <n> <bits>" per case, "FAIL ..." on a mismatch.
//   compact_harness decode < in   "n log_n p bits count", sk[n], words[count][W] (decimal) -> one message per line
#include <cstdio>
#include <cstring>
#include <iostream>
#include <random>
#include <vector>

#include "../../tfhe_fbs_map_amd/csrc/fbs_compact.hpp"
#include "../../tfhe_fbs_map_amd/csrc/fbs_internal.hpp"

using namespace fbs;

static bool make_ctx(fbs_ctx &ctx, uint32_t n, uint32_t log_n, uint32_t p) {
    fbs_params prm{};
    prm.n = n, prm.log_n_poly = log_n, prm.k = 1, prm.l_bsk = 2, prm.beta_bsk = 9, prm.t_ksk = 5, prm.gamma_ksk = 3, prm.p_msg = p;
    prm.sigma_lwe = 1 << 8, prm.sigma_glwe = 1 << 4, prm.bsk_group = 1;
    if (host_ctx_init(&ctx, &prm, 3, nullptr) != FBS_OK) {
        printf("FAIL host_ctx_init: %s\n", ctx.err.c_str());
        return false;
    }
    return true;
}

static int mode_roundtrip() {
    std::mt19937_64 rng(12345);
    int failures = 0;
    const uint32_t ns[] = {1, 12, 63, 64, 127, 734, 766};
    const uint32_t log_ns[] = {8, 10, 11};
    const uint32_t ps[] = {2, 7, 15, 31};
    for (uint32_t n : ns)
        for (uint32_t log_n : log_ns) {
            const uint32_t p = ps[rng() % 4];
            fbs_ctx ctx;
            if (!make_ctx(ctx, n, log_n, p)) return 1;
            ctx.sk_lwe.assign(n, 0);
            for (auto &b : ctx.sk_lwe) b = rng() & 1;
            ctx.sk_glwe.assign(ctx.D, 0);
            for (uint32_t bits = log_n + 1; bits <= 31; bits++) {
                const uint32_t W = compact_words(n, bits), mask = (1u << bits) - 1u;
                const size_t count = 1 + rng() % 9;
                std::vector<int64_t> msgs(count), back(count, -1);
                std::vector<uint64_t> words(count * W);
                for (size_t c = 0; c < count; c++) {
                    msgs[c] = (int64_t)(rng() % (2 * p));
                    std::vector<uint32_t> f(n + 1);
                    uint32_t sum = 0;
                    for (uint32_t i = 0; i < n; i++) {
                        f[i] = (uint32_t)rng() & mask;
                        if (ctx.sk_lwe[i]) sum += f[i];
                    }
                    // body: the message's box centre plus noise well inside half a box
                    const uint64_t centre = (((uint64_t)msgs[c] << bits) + p) / (2 * p);
                    const int64_t half_box = (int64_t)((1ull << bits) / (8 * p));
                    const int64_t noise = half_box ? (int64_t)(rng() % (2 * half_box + 1)) - half_box : 0;
                    f[n] = (uint32_t)(sum + centre + (uint64_t)noise) & mask;
                    for (uint32_t j = 0; j < W; j++) words[c * W + j] = compact_word(j, n + 1, bits, [&](uint32_t i) { return f[i]; });
                    // the unpacking is the packing's inverse, and the bits past the last field are zero
                    for (uint32_t i = 0; i <= n; i++)
                        if (compact_field(words.data() + c * W, i, bits) != f[i]) {
                            printf("FAIL field %u n=%u bits=%u\n", i, n, bits);
                            failures++;
                        }
                    const uint64_t used = (uint64_t)(n + 1) * bits;
                    if (used % 64 && (words[c * W + W - 1] >> (used % 64)) != 0) {
                        printf("FAIL padding n=%u bits=%u\n", n, bits);
                        failures++;
                    }
                }
                host_decrypt_compact(&ctx, words.data(), count, bits, back.data());
                if (back != msgs) {
                    printf("FAIL decode n=%u log_n=%u bits=%u p=%u\n", n, log_n, bits, p);
                    failures++;
                }
                // constant outputs: the compaction of the trivial ciphertext reads back as host_decrypt of that ciphertext
                for (int64_t m = -1; m <= 2 * (int64_t)p; m++) {
                    std::vector<uint64_t> triv(ctx.D + 1, 0), packed(W);
                    triv[ctx.D] = fq_mul(fq_from_i64(m), 2 * ctx.delta_half);
                    int64_t want = 0, got = 0;
                    host_decrypt(&ctx, triv.data(), 1, &want);
                    host_compact_trivial(&ctx, triv[ctx.D], bits, packed.data());
                    host_decrypt_compact(&ctx, packed.data(), 1, bits, &got);
                    for (uint32_t i = 0; i < n; i++)
                        if (compact_field(packed.data(), i, bits)) want = -999;   // mask fields must be zero
                    if (got != want) {
                        printf("FAIL trivial m=%lld n=%u bits=%u p=%u: %lld != %lld\n", (long long)m, n, bits, p, (long long)got, (long long)want);
                        failures++;
                    }
                }
                host_decrypt_compact(&ctx, nullptr, 0, bits, nullptr);   // count = 0 touches nothing
                printf("ok %u %u\n", n, bits);
            }
        }
    return failures ? 1 : 0;
}

static int mode_decode() {
    unsigned long long n, log_n, p, bits, count;
    if (!(std::cin >> n >> log_n >> p >> bits >> count)) return 2;
    fbs_ctx ctx;
    if (!make_ctx(ctx, (uint32_t)n, (uint32_t)log_n, (uint32_t)p)) return 1;
    ctx.sk_lwe.assign(n, 0);
    for (auto &b : ctx.sk_lwe) std::cin >> b;
    const size_t W = compact_words((uint32_t)n, (uint32_t)bits);
    std::vector<uint64_t> words(count * W);
    for (auto &w : words) std::cin >> w;
    if (!std::cin) return 2;
    std::vector<int64_t> msgs(count);
    host_decrypt_compact(&ctx, words.data(), count, (uint32_t)bits, msgs.data());
    for (int64_t m : msgs) printf("%lld\n", (long long)m);
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && !strcmp(argv[1], "roundtrip")) return mode_roundtrip();
    if (argc >= 2 && !strcmp(argv[1], "decode")) return mode_decode();
    fprintf(stderr, "usage: compact_harness roundtrip | decode < input\n");
    return 2;
}

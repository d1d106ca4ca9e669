// Sanitizer harness for the HOST side of libfbsexec ("race detection / sanitizers" -- on the CPU build only; the
// GPU pool has no AddressSanitizer).  Built by tests/c/Makefile with g++ -fsanitize=address,undefined from the product's own
// sources -- csrc/fbs_plan.cpp (the program loader's scheduling, slot reuse and level-index construction), csrc/fbs_host.cpp
// (key generation, encryption, decryption, test vectors, the seeded path, the check of imported keys) and csrc/fbs_select.cpp
// (parameter admission, kernel selection) -- and driven by tests/test_sanitizers.py, tests/test_select.py and
// tests/test_seeded_abi.py.  No GPU, no HIP call.
//
//   host_harness plan  < description        the plan of a program (plain and with shared rotations), EXECUTED in the clear on
//                                           wire slots exactly as the level kernels index them; prints the outputs
//   host_harness crypto                     keygen / encrypt / decrypt / test vectors / imported-key check at toy parameter sets,
//                                           checked
//   host_harness seeded                     the seeded keys and inputs at toy parameter sets, checked (mode_seeded)
//   host_harness select < cases             per line "n log_n k l beta t gamma p group cu_count count [knob=value ...]": the
//                                           launches a key switch and a blind rotation of `count` make, one per line
//                                           ("ks" or "br", kernel name, first bootstrap, count, tab-separated), or "error" and the
//                                           code fbs_ctx_create refuses the set with; a blank line after each case
//
// description (text, whitespace separated): n_inputs n_instr n_terms n_outputs n_tables T
//   kind[n_instr] arg0[n_instr] arg1[n_instr] const[n_instr] term_coef[n_terms] term_src[n_terms] out_wire[n_outputs]
//   per table: len values...      fusable[n_tables]      inputs[n_inputs][T]
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../../tfhe_fbs_map_amd/csrc/fbs_chacha.hpp"
#include "../../tfhe_fbs_map_amd/csrc/fbs_internal.hpp"
#include "../../tfhe_fbs_map_amd/csrc/fbs_plan.hpp"

using namespace fbs;

struct Set {
    uint32_t n, log_n, k, l, beta, t, gamma, p, group;
};

template <class T>
static std::vector<T> read_n(size_t n) {
    std::vector<T> v(n);
    for (auto &x : v) {
        long long tmp;
        if (!(std::cin >> tmp)) {
            fprintf(stderr, "short input\n");
            exit(2);
        }
        x = (T)tmp;
    }
    return v;
}

// Execute a plan in the clear: values live in wire SLOTS [n_slots][T]; a level's linear combinations run sub-stage by sub-stage,
// then its bootstraps read their source's slot and write their own -- every index the level kernels would use is used here, on
// vectors the sanitizer guards.  A slot that is read must hold the wire the description says (`holds`): a wrong reuse aborts.
static int run_plan(const fbs_program_desc &d, const ProgramPlan &plan, const std::vector<std::vector<int64_t>> &tables, size_t T,
                    const std::vector<int64_t> &inputs, std::vector<int64_t> *outputs) {
    std::vector<int64_t> wires((size_t)plan.n_slots * T, -777);
    for (uint32_t i = 0; i < d.n_inputs; i++)
        for (size_t s = 0; s < T; s++) wires.at((size_t)plan.in_slot.at(i) * T + s) = inputs.at((size_t)i * T + s);
    for (uint32_t L = 0; L <= plan.depth; L++) {
        for (const LinPlan &h : plan.lin.at(L)) {
            std::vector<int64_t> fresh(h.dst.size() * T);
            for (size_t o = 0; o < h.dst.size(); o++)
                for (size_t s = 0; s < T; s++) {
                    int64_t acc = h.consts.at(o);
                    for (uint32_t t = h.off.at(o); t < h.off.at(o + 1); t++) acc += h.coefs.at(t) * wires.at((size_t)h.srcs.at(t) * T + s);
                    fresh[o * T + s] = acc;
                }
            for (size_t o = 0; o < h.dst.size(); o++)      // (a stage reads before it writes: k_lincomb's outputs never feed its own inputs)
                for (size_t s = 0; s < T; s++) wires.at((size_t)h.dst.at(o) * T + s) = fresh[o * T + s];
        }
        if (L == plan.depth) break;
        const BootPlan &b = plan.boot.at(L);
        if (b.source_of.size() != b.dst.size() || b.table.size() != b.dst.size()) return 3;
        std::vector<std::vector<int64_t>> shared(b.n_shared, std::vector<int64_t>(T));
        std::vector<int64_t> fresh(b.dst.size() * T);
        for (size_t g = 0; g < b.dst.size(); g++)
            for (size_t s = 0; s < T; s++) {
                const int64_t x = wires.at((size_t)b.src_slot.at(b.source_of.at(g)) * T + s);
                if (b.dst[g] & 0x80000000u) {
                    if (b.table[g] != tables.size()) return 4;                 // a shared rotation starts from TV_0
                    shared.at(b.dst[g] & 0x7FFFFFFFu)[s] = x;                  // (in the clear the accumulator "is" the source value)
                } else {
                    const auto &tab = tables.at(b.table[g]);
                    if (x < 0 || (size_t)x >= tab.size()) return 5;
                    fresh[g * T + s] = tab[(size_t)x];
                }
            }
        for (size_t g = 0; g < b.dst.size(); g++)
            if (!(b.dst[g] & 0x80000000u))
                for (size_t s = 0; s < T; s++) wires.at((size_t)b.dst[g] * T + s) = fresh[g * T + s];
        for (size_t e = 0; e < b.x_row.size(); e++) {
            if (b.x_gate.at(e) >= b.dst.size() || b.dst[b.x_gate[e]] != (0x80000000u | b.x_row[e])) return 6;
            for (size_t s = 0; s < T; s++) {
                const int64_t x = shared.at(b.x_row[e])[s];
                const auto &tab = tables.at(b.x_table.at(e));
                if (x < 0 || (size_t)x >= tab.size()) return 7;
                wires.at((size_t)b.x_dst.at(e) * T + s) = tab[(size_t)x];
            }
        }
    }
    outputs->assign((size_t)d.n_outputs * T, 0);
    for (uint32_t o = 0; o < d.n_outputs; o++)
        for (size_t s = 0; s < T; s++)
            (*outputs)[o * T + s] = plan.out_slot.at(o) >= 0 ? wires.at((size_t)plan.out_slot[o] * T + s) : -1 - plan.out_slot[o];
    return 0;
}

static int mode_plan() {
    const auto head = read_n<uint32_t>(6);
    fbs_program_desc d{};
    d.n_inputs = head[0], d.n_instr = head[1], d.n_terms = head[2], d.n_outputs = head[3];
    const uint32_t n_tables = head[4];
    const size_t T = head[5];
    const auto kind = read_n<uint8_t>(d.n_instr);
    const auto arg0 = read_n<uint32_t>(d.n_instr), arg1 = read_n<uint32_t>(d.n_instr);
    const auto cst = read_n<int64_t>(d.n_instr), tc = read_n<int64_t>(d.n_terms);
    const auto ts = read_n<uint32_t>(d.n_terms);
    const auto ow = read_n<int64_t>(d.n_outputs);
    std::vector<std::vector<int64_t>> tables(n_tables);
    for (auto &t : tables) t = read_n<int64_t>(read_n<uint32_t>(1)[0]);
    const auto fusable = read_n<uint8_t>(n_tables);
    const auto inputs = read_n<int64_t>((size_t)d.n_inputs * T);
    d.kind = kind.data(), d.arg0 = arg0.data(), d.arg1 = arg1.data(), d.const_coef = cst.data(), d.term_coef = tc.data(), d.term_src = ts.data();
    d.out_wire = ow.data();
    std::vector<int64_t> first;
    for (int fused = 0; fused < 2; fused++) {
        ProgramPlan plan;
        std::string err;
        const int rc = plan_program(&d, n_tables, fused ? fusable.data() : nullptr, &plan, &err);
        if (rc != FBS_OK) {
            printf("error %d %s\n", rc, err.c_str());
            return 0;
        }
        std::vector<int64_t> outs;
        const int bad = run_plan(d, plan, tables, T, inputs, &outs);
        if (bad) {
            printf("plan is inconsistent (%d)\n", bad);
            return 1;
        }
        if (fused && outs != first) {
            printf("the plan with shared rotations computes something else\n");
            return 1;
        }
        if (!fused) first = outs;
        printf("%s depth %u slots %u wires %u bootstraps %u keyswitches %u rotations %u max_width %u max_sources %u max_shared %u\n", fused ? "fused" : "plain",
               plan.depth, plan.n_slots, plan.n_wires, plan.n_bootstrap, plan.n_keyswitch, plan.n_rotations, plan.max_width, plan.max_sources, plan.max_shared);
        printf("widths");
        for (const BootPlan &b : plan.boot) printf(" %zu", b.dst.size());
        printf("\n");
    }
    printf("outputs");
    for (int64_t v : first) printf(" %lld", (long long)v);
    printf("\n");
    return 0;
}

static int mode_crypto() {
    const Set sets[] = {{12, 8, 1, 3, 7, 8, 2, 7, 1}, {10, 9, 1, 2, 9, 5, 3, 15, 1}, {12, 8, 1, 1, 20, 8, 2, 7, 2}, {8, 8, 2, 1, 21, 8, 2, 7, 2}};
    for (const Set &s : sets) {
        fbs_ctx ctx;
        fbs_params p{};
        p.n = s.n, p.log_n_poly = s.log_n, p.k = s.k, p.l_bsk = s.l, p.beta_bsk = s.beta, p.t_ksk = s.t, p.gamma_ksk = s.gamma, p.p_msg = s.p;
        p.sigma_lwe = 1 << 8, p.sigma_glwe = 1 << 4, p.bsk_group = s.group;
        if (host_ctx_init(&ctx, &p, 7, nullptr) != FBS_OK) {
            printf("host_ctx_init failed: %s\n", ctx.err.c_str());
            return 1;
        }
        host_keygen(&ctx);
        const uint32_t D = ctx.D;
        if (ctx.sk_lwe.size() != p.n || ctx.sk_glwe.size() != D || ctx.bsk.size() != ctx.n_ggsw * ctx.rows * (p.k + 1) * ctx.N ||
            ctx.ksk.size() != (size_t)D * p.t_ksk * (p.n + 1)) {
            printf("key sizes\n");
            return 1;
        }
        const size_t count = 37;
        std::vector<int64_t> msgs(count), back(count);
        for (size_t i = 0; i < count; i++) msgs[i] = (int64_t)(i % (2 * p.p_msg));
        std::vector<uint64_t> cts(count * (D + 1));
        host_encrypt(&ctx, msgs.data(), count, 1000, cts.data());
        host_decrypt(&ctx, cts.data(), count, back.data());
        if (back != msgs) {
            printf("decrypt(encrypt(m)) != m\n");
            return 1;
        }
        // test vectors: a table on the half torus, the three negacyclic modes, a multi-valued one; one that must be refused
        const std::vector<std::vector<int32_t>> good = {{0, 1, 1, 0, 1, 0, 0}, {0, 1, 1, 0, 1, 0, 0, 1, 0, 0, 1, 0, 1, 1}, {0, 0, 1, 0, 0, 0, 0, 0, 0}, {1, 1, 0, 1, 1, 1, 1, 1, 1}, {0, 1, 2, 3, 2, 1, 0}};
        for (const auto &tab : good) {
            if (tab.size() > 2 * p.p_msg) continue;
            std::vector<uint64_t> tv(ctx.N);
            uint64_t post = 0, d2 = 0, g2 = 0, abs_sum = 0;
            std::vector<uint32_t> pos(p.p_msg + 1);
            std::vector<int32_t> val(p.p_msg + 1);
            uint32_t nd = 0;
            if (host_build_tv(&ctx, tab.data(), (uint32_t)tab.size(), tv.data(), &post) != FBS_OK ||
                host_build_tv_diff(&ctx, tab.data(), (uint32_t)tab.size(), pos.data(), val.data(), &nd, &d2, &g2, &abs_sum) != FBS_OK || nd > p.p_msg + 1) {
                printf("test vector of a valid table refused\n");
                return 1;
            }
        }
        const std::vector<int32_t> bad = {0, 1, 1, 0, 1, 0, 0, 1, 1};      // table[1] + table[1 + p] is not the constant of the overlap (p = 7)
        std::vector<uint64_t> tv(ctx.N);
        uint64_t post = 0;
        if (p.p_msg == 7 && host_build_tv(&ctx, bad.data(), (uint32_t)bad.size(), tv.data(), &post) != FBS_E_TABLE) {
            printf("an invalid table was accepted\n");
            return 1;
        }
        printf("set n=%u N=%u k=%u l=%u group=%u ok\n", p.n, ctx.N, p.k, p.l_bsk, ctx.group);

        // fbs_import_keys's check, on a secret of exactly n words in its own heap block (at two key bits per step the samples
        // run to 3n/2 - 1: only their key-bit pairs may be read), then on a bootstrapping key with one word changed
        std::unique_ptr<uint64_t[]> sk(new uint64_t[p.n]);
        std::copy(ctx.sk_lwe.begin(), ctx.sk_lwe.end(), sk.get());
        if (const char *why = imported_keys_mismatch(&ctx, sk.get(), ctx.sk_glwe.data(), ctx.bsk.data(), ctx.ksk.data())) {
            printf("generated keys refused: %s\n", why);
            return 1;
        }
        std::vector<uint64_t> bsk = ctx.bsk;
        bsk[(size_t)p.k * ctx.N + 1] = fq_add(bsk[(size_t)p.k * ctx.N + 1], FQ / 2);   // sample 0, row 0, body coefficient 1
        const char *why = imported_keys_mismatch(&ctx, sk.get(), ctx.sk_glwe.data(), bsk.data(), ctx.ksk.data());
        if (!why || strncmp(why, "bootstrapping key", 17) != 0) {
            printf("a changed bootstrapping key was accepted\n");
            return 1;
        }
        printf("import check n=%u N=%u k=%u l=%u group=%u ok\n", p.n, ctx.N, p.k, p.l_bsk, ctx.group);
    }
    return 0;
}

// ---- seeded mode: the host side of the seeded path (host_keygen_seeded, host_expand_seeded_keys, host_encrypt_seeded,
// host_expand_seeded).  At toy parameter sets (k = 1, 2, 3; bsk_group 1 and 2; l = 1 and 2) it checks, and prints "<set> ok" per set:
//   * every row of the seeded keys has the phase the fbs_key_sizes layout says it encrypts, plus exactly the noise sample of
//     its seeded noise stream;
//   * expanding (mask key, bodies) reproduces the generated keys word for word;
//   * the noise of every seeded row differs from that of the matching fbs_keygen row (stream separation);
//   * the mask key is the first 32 bytes of block 0 of stream (DOM_MASK_KEY, 0), and changing one of its bytes changes every
//     expanded mask;
//   * seeded ciphertexts expand and decrypt to their messages, with the noise of their stream.
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

static int seeded_set(const Set &s) {
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

static int mode_seeded() {
    const Set sets[] = {{12, 8, 1, 2, 9, 8, 2, 7, 1}, {12, 8, 1, 1, 20, 6, 3, 7, 2}, {8, 8, 2, 1, 21, 8, 2, 7, 2},
                        {10, 8, 2, 2, 10, 5, 3, 15, 1}, {8, 8, 3, 1, 18, 4, 4, 7, 2}, {6, 8, 3, 2, 9, 3, 5, 7, 1}};
    for (const Set &s : sets) {
        if (seeded_set(s)) continue;
        printf("k=%u l=%u group=%u ok\n", s.k, s.l, s.group);
    }
    return failures ? 1 : 0;
}

static int mode_select() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.find_first_not_of(" \t") == std::string::npos) continue;
        std::istringstream in(line);
        fbs_params p{};
        long long cus = 0, count = 0;
        if (!(in >> p.n >> p.log_n_poly >> p.k >> p.l_bsk >> p.beta_bsk >> p.t_ksk >> p.gamma_ksk >> p.p_msg >> p.bsk_group >> cus >> count) ||
            cus < 1 || count < 0) {
            fprintf(stderr, "bad case: %s\n", line.c_str());
            return 2;
        }
        p.sigma_lwe = 1 << 8, p.sigma_glwe = 1 << 4;
        fbs_ctx ctx;
        int rc = host_ctx_init(&ctx, &p, 1, nullptr);
        if (rc == FBS_OK) rc = check_kernel_built(&ctx);   // (what fbs_ctx_create refuses)
        if (rc != FBS_OK) {
            printf("error\t%d\n\n", rc);
            continue;
        }
        ctx.cu_count = (int)cus;
        for (std::string kv; in >> kv;) {
            const size_t eq = kv.find('=');
            int64_t *slot = eq == std::string::npos ? nullptr : tune_knob(ctx.tune, kv.substr(0, eq));
            if (!slot) {
                fprintf(stderr, "bad knob: %s\n", kv.c_str());
                return 2;
            }
            *slot = atoll(kv.c_str() + eq + 1);
        }
        for (const Launch &l : select_keyswitch(&ctx, (size_t)count))
            printf("ks\t%s\t%zu\t%zu\n", kernel_name(l.kernel).c_str(), l.first, l.count);
        for (const Launch &l : select_blind_rotate(&ctx, (size_t)count))
            printf("br\t%s\t%zu\t%zu\n", kernel_name(l.kernel).c_str(), l.first, l.count);
        printf("\n");
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && !strcmp(argv[1], "plan")) return mode_plan();
    if (argc >= 2 && !strcmp(argv[1], "crypto")) return mode_crypto();
    if (argc >= 2 && !strcmp(argv[1], "select")) return mode_select();
    if (argc >= 2 && !strcmp(argv[1], "seeded")) return mode_seeded();
    fprintf(stderr, "usage: host_harness plan|crypto|select|seeded\n");
    return 2;
}

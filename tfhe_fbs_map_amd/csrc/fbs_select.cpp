// Kernel selection (fbs_select.hpp): host code only.  The measurements behind each rule are in the comments here and in DESIGN.md.
#include "fbs_select.hpp"

#include <algorithm>
#include <cmath>

#include "fbs_internal.hpp"

namespace fbs {

namespace {

// bootstraps per CU up to which a k = 1 launch takes the one-bootstrap-per-CU kernel, and a k = 2 launch the twelve-wave shape
constexpr size_t CU_MAX_PER_CU = 2, K2_CU_ROUNDS = 3;

// the blind-rotation kernels by parameter shape
enum class Path { GLWE, K2, PAIRS, GENERIC };

Path path_of(const fbs_ctx *ctx) {
    const fbs_params &p = ctx->p;
    // k = 2 at N = 1024 with two key bits per step and one level has kernels of its own; every other k >= 2 the general GLWE kernel
    if (p.k == 2 && p.log_n_poly == 10 && ctx->group == 2 && p.l_bsk == 1) return Path::K2;
    if (p.k >= 2) return Path::GLWE;
    return ctx->group == 2 ? Path::PAIRS : Path::GENERIC;
}

// DIG of k_blind_rotate: the digit form of the gadget decomposition (l > 5: generic; l = 1: 4; l = 2: 4 + by_beta; else by_beta)
int generic_dig(const fbs_params &p) {
    const int by_beta = p.beta_bsk <= 7 ? 3 : p.beta_bsk <= 9 ? 2 : 1;
    return p.l_bsk > 5 ? 0 : p.l_bsk == 1 ? 4 : p.l_bsk == 2 ? 4 + by_beta : by_beta;
}

bool cu_built(int log_n, int nl, int first) {
#define X(L, NL, FIRST, LEAN) \
    if (log_n == L && nl == NL && first == FIRST) return true;
    FBS_CU_KERNELS(X)
#undef X
    return false;
}

// The whole-round cut of a launch: a launch longer than `per_round` bootstraps whose last round would hold at most `max_rest`
// runs the whole rounds first and the rest as a launch of its own, in the shape its size asks for.
struct Rounds {
    size_t per_round = 0, max_rest = 0;   // max_rest = 0: never cut
};

Rounds rounds_of(const fbs_ctx *ctx) {
    const fbs_params &p = ctx->p;
    const size_t cus = (size_t)ctx->cu_count;
    switch (path_of(ctx)) {
    case Path::GLWE: {
        // rest of at most two bootstraps per CU (one where the throughput shape holds two): k = 3, N = 512: 1 024 = 768 + 256
        // bootstraps in 4.1 + 1.8 ms against two rounds' 7.4
        const size_t full = (size_t)glwe_full_fpw(p.log_n_poly, p.k);
        return {full * cus, ctx->tune.br_glwe_fpw == 0 ? (full > 2 ? 2 : 1) * cus : 0};
    }
    case Path::K2:
        // rounds of four-bootstrap workgroups, a rest the twelve-wave shape takes: 1 124 = 1 024 + 100 in 7.3 + 2.1 ms against
        // two rounds' 14.5
        return {4 * cus, ctx->tune.br_k2_shape == 0 && ctx->tune.br_cu_kernel ? K2_CU_ROUNDS * cus : 0};
    case Path::GENERIC:
        // the benchmark shape (below): whole rounds when the last one is far from full -- a partly filled round is faster as small
        // workgroups (768 bootstraps 8.2 ms against 9.3)
        if (p.log_n_poly == 10 && generic_dig(p) == 3) return {4 * cus, (7 * 4 * cus - 1) / 8};
        return {};
    case Path::PAIRS: return {};
    }
    return {};
}

// the kernel of one launch of `n` bootstraps (after the cut)
Kernel pick_blind_rotate(const fbs_ctx *ctx, size_t n) {
    const fbs_params &p = ctx->p;
    const Tune &tune = ctx->tune;
    const int L = (int)p.log_n_poly;
    const size_t cus = (size_t)ctx->cu_count;
    switch (path_of(ctx)) {
    case Path::GLWE: {
        // k + 1 waves per bootstrap (fbs_blind_rotate_glwe.hip); bootstraps per workgroup by launch size: one up to one
        // bootstrap per CU, two up to two, the throughput shape beyond (glwe_full_fpw); br_glwe_fpw: 1, 2, larger = throughput
        const int full = glwe_full_fpw(p.log_n_poly, p.k);
        int fpw = (int)tune.br_glwe_fpw;
        if (fpw == 0) fpw = n <= cus ? 1 : (n <= 2 * cus && full > 2) ? 2 : full;
        fpw = fpw == 1 ? 1 : fpw == 2 ? std::min(full, 2) : full;
        return {Family::GLWE, {L, (int)p.k + 1, (int)ctx->group, fpw}, false};
    }
    case Path::K2: {
        // br_k2_shape: 0 = by launch size; 3 = always three waves per bootstrap; 12 = always the twelve-wave shape.
        // Launches of up to three bootstraps per CU: one bootstrap on twelve waves, round after round (n = 734, one box: 2.06 ms
        // at 64, 2.36 at 256, 4.43 at 512, 6.37 at 768 bootstraps against 3.33 / 3.49 / 4.92 / 6.79 on three waves per
        // bootstrap; from 769 on a round of four-bootstrap workgroups is ahead: 6.8-7.2 ms up to 1 024)
        const int64_t shape = tune.br_k2_shape;
        if (shape == 12 || (shape == 0 && n <= K2_CU_ROUNDS * cus && tune.br_cu_kernel)) return {Family::CU_K2, {}, false};
        // three waves per bootstrap: up to one bootstrap per CU one per workgroup; up to two: two; beyond: four (tools/k2_check.py)
        return {Family::PAIRS_K2, {10, n <= cus ? 1 : n <= 2 * cus ? 2 : 4}, false};
    }
    case Path::PAIRS:
        // launches of at most one bootstrap per CU: the whole-CU shape (2.65-2.9 ms per bootstrap against 3.3-3.4; two rounds of
        // it are no faster than two bootstraps side by side in the four-wave kernel: 5.44 against 5.35 ms per 512).  Two gadget
        // levels (the 128-bit sets for p = 31): the whole-CU shape for every launch, round after round -- the two-waves-per-
        // polynomial kernel spills 100 registers there (22.7 ms per 1024 bootstraps against 17.1)
        if ((n <= cus || p.l_bsk == 2) && L == 11 && p.l_bsk <= 2 && tune.br_cu_kernel && small_key_needed(ctx))
            return {Family::CU_PAIRS, {11, (int)p.l_bsk}, false};
        return {Family::PAIRS, {L, lanes_log2_for(L), p.l_bsk == 1 ? 4 : p.beta_bsk <= 7 ? 3 : 0}, false};
    case Path::GENERIC: break;
    }
    const int dig = generic_dig(p);
    const bool small_key = small_key_needed(ctx);
    // Launches that leave most of the chip empty: one bootstrap on the eight waves of a CU (fbs_blind_rotate_cu.hip).  Up to TWO
    // bootstraps per CU: the second round of workgroups follows the first CU by CU (512 bootstraps: 5.9 ms against 6.5 ms for
    // two bootstraps side by side in the two-waves-per-bootstrap kernel; 384: 6.0 against 6.5).  Beyond that the small
    // workgroups of k_blind_rotate win (768: 8.3 ms against three rounds of 2.95).
    const int first = p.beta_bsk <= 7 ? 2 : p.beta_bsk <= 9 ? 1 : 0;
    if (small_key && n <= CU_MAX_PER_CU * cus && tune.br_cu_kernel && cu_built(L, (int)p.l_bsk, first)) {
        // more than one bootstrap per CU: the two-workgroups-per-CU variant where there is one (N = 1024, up to three levels)
        // (512 bootstraps at P1024: 6.07 ms as two rounds of the 162-register kernel, 5.40 ms with two workgroups per CU; 1 536 =
        // 1 024 + 512: 99.7 -> 105.3 k FBS/s)
        const bool lean = L == 10 && p.l_bsk <= 3 && (tune.br_cu_lean == 2 || (tune.br_cu_lean == 1 && n > cus));
        return {Family::CU, {L, (int)p.l_bsk, first}, lean};
    }
    // The benchmark shape: four bootstraps = the eight waves of a CU in one workgroup, for whole rounds and rounds that are
    // (nearly) full.  One workgroup per CU holds ALL the waves a CU holds in one barrier domain: the two waves that share a SIMD
    // then advance in lockstep; as separate workgroups the SIMD's oldest-first arbitration lets one of them run ahead (measured
    // per workgroup with the wall clock, P1024: 6.0 ms for the favoured ones, 10.7 ms for the others, every XCD alike), and once
    // the favoured half has left, the rest runs with one wave per SIMD and nothing to cover its stalls: 10.7 ms per 1024-batch
    // against 10.0 ms in lockstep.  It pays when the launch fills whole rounds (a round = what the chip holds at once: 600
    // bootstraps take 9.1 ms as small workgroups, 10.05 ms as whole-CU ones); beyond a few rounds the hardware refills freed
    // slots anyway.  Measured and NOT adopted for the other shapes: two-level sets at N = 1024 (slower with the priority
    // hand-over: 152.5 against 155.5 k FBS/s at p = 2, 124 against 131 k at p = 4), N = 2048 with two bootstraps per workgroup
    // (pairs 10.13 against 9.94 ms, l = 2 23.1 against 21.7 ms; with the priority hand-over as well: 10.34 against 9.87 ms at
    // 1024 bootstraps, 82.4 against 73.7 ms at 8192 -- the transforms' own barriers then span eight waves).
    if (L == 10 && dig == 3) {
        const size_t per_round = 4 * cus, r = n % per_round;
        if (r == 0 || 8 * r >= 7 * per_round) return {Family::BLIND_ROTATE, {10, 6, 3, 4}, false};
    }
    // the two-level 128-bit sets at N = 1024 in launches of more than two rounds: no taking turns (see TURNS)
    if (L == 10 && (dig == 6 || dig == 7) && n > 8 * cus) return {Family::BLIND_ROTATE, {10, 6, dig, 1}, true};
    // at most one bootstrap per CU: the shape with twice the waves per bootstrap, where there is one (fbs_ntt.hpp)
    if (small_key && n <= cus) return {Family::BLIND_ROTATE, {L, lanes_log2_for_small_launch(L), dig, 1}, false};
    // Two bootstraps per workgroup exactly where two-wave workgroups would double up on half of the SIMDs: between one and two
    // bootstraps per CU (measured per 1024-coefficient launch: 6.5 ms against 9.8).  Up to one per CU the two-wave form is
    // faster (5.7 against 6.5 ms), beyond two per CU too (9.8-11.1 against 11.1).
    const bool pair = lanes_log2_for(L) == 6 && n > cus && n <= 2 * cus;
    return {Family::BLIND_ROTATE, {L, lanes_log2_for(L), dig, pair ? 2 : 1}, false};
}

std::string args(const int *t, int n) {
    std::string s;
    for (int i = 0; i < n; i++) s += (i ? "," : "") + std::to_string(t[i]);
    return s;
}

}  // namespace

std::vector<Launch> select_blind_rotate(const fbs_ctx *ctx, size_t count) {
    if (count == 0) return {};
    const Rounds r = rounds_of(ctx);
    const size_t rest = r.per_round ? count % r.per_round : 0;
    const size_t head = count > r.per_round && rest != 0 && rest <= r.max_rest ? count - rest : count;
    std::vector<Launch> out{{pick_blind_rotate(ctx, head), 0, head}};
    if (head < count) out.push_back({pick_blind_rotate(ctx, count - head), head, count - head});
    return out;
}

bool ks_gemm_exact(const fbs_ctx *ctx) {
    // the operands: balanced digits in [-2^(gamma-1), 2^(gamma-1)) are stored as int8 (k_ks_digits), which holds them up to gamma = 8;
    // the sums: |digit| * |limb| * kN t <= 2^(gamma-1) 2^7 kN t in an int32
    return ctx->p.gamma_ksk <= 8 && std::ldexp((double)ctx->D * ctx->p.t_ksk, (int)ctx->p.gamma_ksk + 6) < 2147483648.0;
}

std::vector<Launch> select_keyswitch(const fbs_ctx *ctx, size_t count) {
    if (count == 0) return {};
    const fbs_params &p = ctx->p;
    Kernel k;
    // The int8 GEMM on the matrix cores serves every batch size (round 2 used it above 64 ciphertexts only; below, the integer
    // kernels took 0.54 ms for 32-64 ciphertexts and 2.7 ms for 1-16, the GEMM takes 0.04-0.06 ms: its cost is streaming the
    // key's 31 MB of limb fragments, whatever the number of rows).
    if (ctx->tune.ks_mfma && ks_gemm_exact(ctx)) {
        k = {Family::KS_GEMM, {2, 2}, false};
    } else if (count < 32) {
        k = {Family::KS_INT, {8}, false};
    } else if (count <= 64) {   // lanes = ciphertexts: pays once a wave is at least half full
        k = {Family::KS_LANES, {8, 1, 4}, false};
    } else {
        // FP64 form: needs room to accumulate at least one mask word exactly
        const double per_word = (double)p.t_ksk * std::ldexp(1.0, 44 + (int)p.gamma_ksk);
        const double room = std::ldexp(1.0, 53) - std::ldexp(1.0, 45);
        if (ctx->tune.ks_fp && per_word <= room) k = {Family::KS_FP, {8, 2, 8}, false};
        else k = {Family::KS_LANES, {8, 2, 8}, false};
    }
    return {{k, 0, count}};
}

std::string kernel_name(const Kernel &k) {
    switch (k.family) {
    case Family::BLIND_ROTATE: return "k_blind_rotate<" + args(k.t, 4) + (k.alt ? ",false>" : ">");
    case Family::PAIRS: return "k_blind_rotate_pairs<" + args(k.t, 3) + ">";
    case Family::CU: return "k_blind_rotate_cu<" + args(k.t, 3) + (k.alt ? ",lean>" : ">");
    case Family::CU_PAIRS: return "k_blind_rotate_cu_pairs<" + args(k.t, 2) + ">";
    case Family::PAIRS_K2: return "k_blind_rotate_pairs_k2<" + args(k.t, 2) + ">";
    case Family::CU_K2: return "k_blind_rotate_cu_k2";
    case Family::GLWE: return "k_blind_rotate_glwe<" + args(k.t, 4) + ">";
    case Family::KS_GEMM: return "k_ks_gemm<" + args(k.t, 2) + "> (int8 MFMA)";
    case Family::KS_FP: return "k_keyswitch_fp<" + args(k.t, 3) + ">";
    case Family::KS_LANES: return "k_keyswitch_lanes<" + args(k.t, 3) + ">";
    case Family::KS_INT: return "k_keyswitch<" + args(k.t, 1) + ">";
    }
    return "?";
}

void kernel_catalog(std::vector<std::string> *out) {
    for (const Kernel &k : {Kernel{Family::KS_GEMM, {2, 2}, false}, Kernel{Family::KS_FP, {8, 2, 8}, false},
                            Kernel{Family::KS_LANES, {8, 2, 8}, false}, Kernel{Family::KS_LANES, {8, 1, 4}, false},
                            Kernel{Family::KS_INT, {8}, false}})
        out->push_back(kernel_name(k));
#define X(L, LL, DIG, FPW, TURNS) out->push_back(kernel_name({Family::BLIND_ROTATE, {L, LL, DIG, FPW}, !(TURNS)}));
    FBS_BR_KERNELS(X)
#undef X
#define X(L, DIG) out->push_back(kernel_name({Family::PAIRS, {L, lanes_log2_for(L), DIG}, false}));
    FBS_PAIRS_KERNELS(X)
#undef X
#define X(L, NL, FIRST, LEAN) out->push_back(kernel_name({Family::CU, {L, NL, FIRST}, LEAN}));
    FBS_CU_KERNELS(X)
#undef X
#define X(L, NL) out->push_back(kernel_name({Family::CU_PAIRS, {L, NL}, false}));
    FBS_CU_PAIRS_KERNELS(X)
#undef X
#define X(L, FPW) out->push_back(kernel_name({Family::PAIRS_K2, {L, FPW}, false}));
    FBS_PAIRS_K2_KERNELS(X)
#undef X
    out->push_back(kernel_name({Family::CU_K2, {}, false}));
    // bootstraps per workgroup 1, 2 and the throughput shape's (listed once where that is 2)
#define X(L, K1)                                                                             \
    for (int g = 1; g <= 2; g++)                                                             \
        for (int fpw = 1; fpw <= glwe_full_fpw(L, K1 - 1); fpw++)                            \
            if (fpw <= 2 || fpw == glwe_full_fpw(L, K1 - 1))                                 \
                out->push_back(kernel_name({Family::GLWE, {L, K1, g, fpw}, false}));
    FBS_GLWE_SHAPES(X)
#undef X
}

bool reads_small_key(const Kernel &k) {
    return k.family == Family::CU || k.family == Family::CU_PAIRS || k.family == Family::CU_K2 ||
           (k.family == Family::BLIND_ROTATE && k.t[1] != lanes_log2_for(k.t[0]));
}

bool small_key_needed(const fbs_ctx *ctx) {
    const fbs_params &p = ctx->p;
    const int L = (int)p.log_n_poly;
    // (two key bits per step: a second copy of the 1.5 times larger key only where a kernel reads it -- N = 2048, l <= 2)
    // (... and N = 1024 at GLWE dimension 2: the whole-workgroup latency shape of fbs_blind_rotate_k2.hip)
    return lanes_log2_for_small_launch(L) != lanes_log2_for(L) &&
           (ctx->group == 1 || (L == 11 && p.l_bsk <= 2) || (L == 10 && p.k == 2));
}

int check_kernel_built(const fbs_ctx *ctx) {
    if (const char *why = kernel_not_built(ctx->p)) return set_error(ctx, FBS_E_INVALID, why);
    return FBS_OK;
}

int64_t *tune_knob(Tune &t, const std::string &k) {
    return k == "ks_mfma" ? &t.ks_mfma : k == "ks_fp" ? &t.ks_fp : k == "br_cu_kernel" ? &t.br_cu_kernel : k == "br_cu_lean" ? &t.br_cu_lean :
           k == "br_k2_shape" ? &t.br_k2_shape : k == "br_glwe_fpw" ? &t.br_glwe_fpw : k == "pack_slices" ? &t.pack_slices :
           k == "keys_on_device" ? &t.keys_on_device : nullptr;
}

}  // namespace fbs

// Which kernel instantiation a launch takes -- host code only, no HIP call (libfbsexec.so builds it, and so does the sanitizer
// harness of tests/c).  select_blind_rotate / select_keyswitch turn a context and a batch size into the launches a call makes,
// each a descriptor (kernel family + template arguments) and a range of bootstraps; the launch files (fbs_blind_rotate*.hip,
// fbs_kernels.hip) map a descriptor to its hipLaunchKernelGGL and decide nothing.  The instantiation lists below are what those
// files instantiate and what fbs_kernel_catalog lists.
#pragma once
#ifndef FBS_HOST_ONLY   // (the client library, libfbsclient.so, is built without HIP)
#include <hip/hip_runtime.h>   // (the attributes of fbs_field.hpp; nothing here calls HIP)
#endif

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/fbs_exec.h"
#include "fbs_field.hpp"

namespace fbs {

struct Tune;

// 2^LL lanes per polynomial of N = 2^log_n coefficients: the main shape, and the shape for launches of at most one bootstrap per
// CU, which has its own copy of the bootstrapping key (fbs_ntt.hpp)
#ifndef FBS_SMALL_LAUNCH_LL_1024
#define FBS_SMALL_LAUNCH_LL_1024 8
#endif
constexpr int lanes_log2_for_small_launch(int log_n) {
    return log_n == 10 ? FBS_SMALL_LAUNCH_LL_1024 : log_n == 11 ? 8 : (log_n <= 10 ? 6 : log_n - 4);
}
#ifdef FBS_COEFS_PER_LANE_LOG2   // experiments: force 2^k coefficients per lane everywhere it is possible
constexpr int lanes_log2_for(int log_n) { return log_n - FBS_COEFS_PER_LANE_LOG2 < 6 ? 6 : log_n - FBS_COEFS_PER_LANE_LOG2; }
#else
constexpr int lanes_log2_for(int log_n) { return log_n <= 10 ? 6 : log_n - 4; }
#endif

// ---- the instantiations (X-macro lists) ---------------------------------------------------------------------------------------
// k_blind_rotate<LOGN, LL, DIG, FPW, TURNS> (fbs_blind_rotate.hip): every digit form on the main shape, also two bootstraps per
// workgroup where a polynomial is one wave, also on the small-launch shape where it differs; the benchmark shape (four per
// workgroup); the two-level N = 1024 sets without taking turns
#define FBS_BR_DIGITS(X, L, LL, FPW)                                                                                            \
    X(L, LL, 0, FPW, true) X(L, LL, 1, FPW, true) X(L, LL, 2, FPW, true) X(L, LL, 3, FPW, true) X(L, LL, 4, FPW, true)          \
    X(L, LL, 5, FPW, true) X(L, LL, 6, FPW, true) X(L, LL, 7, FPW, true)
#define FBS_BR_KERNELS(X)                                                                                                       \
    FBS_BR_DIGITS(X, 8, lanes_log2_for(8), 1) FBS_BR_DIGITS(X, 8, lanes_log2_for(8), 2)                                         \
    FBS_BR_DIGITS(X, 9, lanes_log2_for(9), 1) FBS_BR_DIGITS(X, 9, lanes_log2_for(9), 2)                                         \
    FBS_BR_DIGITS(X, 10, lanes_log2_for(10), 1) FBS_BR_DIGITS(X, 10, lanes_log2_for(10), 2)                                     \
    FBS_BR_DIGITS(X, 10, lanes_log2_for_small_launch(10), 1)                                                                    \
    FBS_BR_DIGITS(X, 11, lanes_log2_for(11), 1) FBS_BR_DIGITS(X, 11, lanes_log2_for_small_launch(11), 1)                       \
    FBS_BR_DIGITS(X, 12, lanes_log2_for(12), 1)                                                                                 \
    X(10, 6, 3, 4, true) X(10, 6, 6, 1, false) X(10, 6, 7, 1, false)
// k_blind_rotate_pairs<LOGN, lanes_log2_for(LOGN), DIG> (two key bits per step)
#define FBS_PAIRS_KERNELS(X) X(10, 4) X(10, 3) X(10, 0) X(11, 4) X(11, 3) X(11, 0) X(12, 4) X(12, 3) X(12, 0)
// k_blind_rotate_cu<LOGN, NL, FIRST, LEAN> (fbs_blind_rotate_cu.hip: N = 1024 with up to four gadget levels, N = 2048 with up to
// two; four levels have at most 7 bits each, l * beta <= 30)
#define FBS_CU_KERNELS(X)                                                                                                       \
    X(10, 1, 0, false) X(10, 1, 0, true) X(10, 1, 1, false) X(10, 1, 1, true) X(10, 1, 2, false) X(10, 1, 2, true)              \
    X(10, 2, 0, false) X(10, 2, 0, true) X(10, 2, 1, false) X(10, 2, 1, true) X(10, 2, 2, false) X(10, 2, 2, true)              \
    X(10, 3, 0, false) X(10, 3, 0, true) X(10, 3, 1, false) X(10, 3, 1, true) X(10, 3, 2, false) X(10, 3, 2, true)              \
    X(10, 4, 2, false)                                                                                                          \
    X(11, 1, 0, false) X(11, 1, 1, false) X(11, 1, 2, false) X(11, 2, 0, false) X(11, 2, 1, false) X(11, 2, 2, false)
// k_blind_rotate_cu_pairs<LOGN, NL> (two key bits per step on a whole CU)
#define FBS_CU_PAIRS_KERNELS(X) X(11, 1) X(11, 2)
// k_blind_rotate_pairs_k2<LOGN, FPW> (fbs_blind_rotate_k2.hip; k_blind_rotate_cu_k2 is not a template)
#define FBS_PAIRS_K2_KERNELS(X) X(10, 1) X(10, 2) X(10, 4)
// k_blind_rotate_glwe<LOGN, K1, GROUP, FPW> (fbs_blind_rotate_glwe.hip) at the shapes (LOGN, K1 = k + 1) below: k = 2, 3, 4 at
// N = 256 and 512, k = 2, 3 at N = 1024; GROUP 1 and 2; FPW 1, 2 and the throughput shape's glwe_full_fpw
#define FBS_GLWE_SHAPES(X) X(8, 3) X(8, 4) X(8, 5) X(9, 3) X(9, 4) X(9, 5) X(10, 3) X(10, 4)

constexpr bool glwe_shape_built(uint32_t log_n, uint32_t k) {   // is there a kernel for GLWE dimension k >= 2 at N = 2^log_n?
#define X(L, K) (log_n == L && k + 1 == K) ||
    return FBS_GLWE_SHAPES(X) false;
#undef X
}

// Bootstraps per workgroup of k_blind_rotate_glwe's THROUGHPUT shape (a full round is glwe_full_fpw x CUs): twelve waves where
// the registers allow three waves per SIMD (N <= 512: 4, 3, 2 bootstraps at k = 2, 3, 4), six to eight at N = 1024.  Launches that
// leave most of the chip empty take ONE bootstrap per workgroup up to one per CU (every wave alone on its SIMD: a step is one wave's
// instruction chain, not three waves' sharing an issue port) and two up to two per CU.  Measured at k = 3, N = 512, n = 614 (the
// 128-bit set for p <= 4), ms per launch: 64 / 256 bootstraps 1.55 / 1.81 with one per workgroup against 3.32 / 3.37 with three;
// 512: 2.90 with two against 3.61; 768: 4.06 with three.  (FOUR per workgroup there -- sixteen waves at 128 registers with 196
// bytes spilled, one set of landing words -- 6.99 against 5.43 ms per 1 024, 20.6 against 14.5 per 3 072.)
constexpr int glwe_full_fpw(uint32_t log_n, uint32_t k) { return !glwe_shape_built(log_n, k) ? 0 : log_n >= 10 ? 2 : 12 / (int)(k + 1); }

// ---- launch descriptors -------------------------------------------------------------------------------------------------------
enum class Family : uint8_t {
    BLIND_ROTATE,   // k_blind_rotate<LOGN, LL, DIG, FPW[, TURNS = false]>
    PAIRS,          // k_blind_rotate_pairs<LOGN, LL, DIG>
    CU,             // k_blind_rotate_cu<LOGN, NL, FIRST[, lean]>
    CU_PAIRS,       // k_blind_rotate_cu_pairs<LOGN, NL>
    PAIRS_K2,       // k_blind_rotate_pairs_k2<LOGN, FPW>
    CU_K2,          // k_blind_rotate_cu_k2
    GLWE,           // k_blind_rotate_glwe<LOGN, K1, GROUP, FPW>
    KS_GEMM,        // k_ks_gemm<2, 2> and the digit / finish kernels around it (int8 MFMA)
    KS_FP,          // k_keyswitch_fp<COLS, CPL, WAVES>
    KS_LANES,       // k_keyswitch_lanes<COLS, CPL, WAVES>
    KS_INT,         // k_keyswitch<FB>
};
struct Kernel {
    Family family;
    int t[4];       // template arguments in the kernel's order (unused: 0)
    bool alt;       // BLIND_ROTATE: TURNS = false; CU: the lean variant
};
struct Launch {
    Kernel kernel;
    size_t first, count;   // bootstraps [first, first + count) of the call (a key switch: its rows)
};

// The launches of a blind rotation of `count` bootstraps, in order: one, or whole rounds and then the rest.  Reads only the host
// fields p, group, cu_count and tune of the context.
std::vector<Launch> select_blind_rotate(const fbs_ctx *ctx, size_t count);
// The launch of a key switch of `count` rows (one: nothing cuts a key switch).  Reads only p, D and tune.
std::vector<Launch> select_keyswitch(const fbs_ctx *ctx, size_t count);
// "k_blind_rotate<10,6,3,4>": the profile tables and fbs_kernel_catalog name an instantiation so
std::string kernel_name(const Kernel &k);
// every instantiation the selection can pick (fbs_kernel_catalog)
void kernel_catalog(std::vector<std::string> *out);
// does the kernel read the second copy of the bootstrapping key (the small-launch evaluation order)?
bool reads_small_key(const Kernel &k);
// does the context need that copy?  (key upload makes it exactly when this says so)
bool small_key_needed(const fbs_ctx *ctx);
// int8 GEMM key switch on the matrix cores: exact while the balanced digits fit an int8 (gamma <= 8) and the int32 sums
// 2^(gamma-1) * 2^7 * kN t stay below 2^31
bool ks_gemm_exact(const fbs_ctx *ctx);
// Parameter admission, in two parts.  The arithmetic limits: null, or why the set is refused.  host_ctx_init asks before it computes
// anything from the gadget parameters (q / 2^(beta (lv + 1)), q / 2^(gamma (v + 1))); D = k N.
inline const char *params_out_of_range(const fbs_params &p, uint64_t D) {
    if (p.l_bsk < 1 || p.beta_bsk < 1 || p.l_bsk * p.beta_bsk > 30 || p.l_bsk * p.beta_bsk > FQ_BITS - 2) return "need 1 <= l*beta <= 30";
    if (p.t_ksk < 1 || p.gamma_ksk < 1 || p.t_ksk * p.gamma_ksk > 31 || p.t_ksk * p.gamma_ksk > FQ_BITS - 2) return "need 1 <= t*gamma <= 31";
    if (p.n < 1 || p.n > 4096) return "need 1 <= n <= 4096";
    // lazy FP64 ranges (fbs_field.hpp): partial external products stay below 2^50 while (k+1)*l <= 20
    if ((p.k + 1) * p.l_bsk > 20) return "need (k+1)*l <= 20";
    // 64-bit key-switch accumulators: D*t digits < 2^gamma times words < 2^46
    const double bits = FQ_BITS + p.gamma_ksk + std::log2((double)p.t_ksk * (double)D);
    if (bits > 63.9 || bits - 32.0 > 31.9) return "key-switch accumulator would overflow";   // whole sum in 64 bits; high-word partial sums in 32
    return nullptr;
}
// ... and whether a kernel is built for the set: null, or why not (fbs_ctx_create of either library asks this after host_ctx_init,
// in admit_params of fbs_api_checks.hpp: a set the GPU library refuses is refused by the client library too) ...
inline const char *kernel_not_built(const fbs_params &p) {
    if (p.k >= 2 && !glwe_shape_built(p.log_n_poly, p.k))
        return "GLWE dimensions k >= 2 are built for k = 2, 3, 4 at N = 256 and 512 and k = 2, 3 at N = 1024";
    if (p.log_n_poly < 8 || p.log_n_poly > 12) return "supported polynomial sizes are N = 256, 512, 1024, 2048, 4096";
    if (p.bsk_group == 2 && p.k == 1 && (p.log_n_poly < 10 || p.l_bsk > 5))
        return "two key bits per step (bsk_group = 2) at k = 1 is built for N = 1024, 2048 and 4096, l <= 5";
    return nullptr;
}
// ... as FBS_OK or FBS_E_INVALID (text in ctx->err).  Kept for the host harness of tests/c/ (select mode), which builds no entry
// file: the libraries ask kernel_not_built themselves, in admit_params.
int check_kernel_built(const fbs_ctx *ctx);
// the fbs_ctx_tune knob `name`, or null
int64_t *tune_knob(Tune &t, const std::string &name);

}  // namespace fbs

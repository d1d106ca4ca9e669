// The rounded-Gaussian noise sample (sampler 1) and the dispatch between it and the Irwin-Hall sample (sampler 0, fbs_chacha.hpp),
// shared by the host (noise_sample, fbs_host.cpp) and the device encryption kernels (fbs_io.hip): both run this code, and it is
// written so that both compute the same bits.
//
// gauss_sample reads the six words that sample idx of a stream owns (words 6 idx .. 6 idx + 5), as irwin_hall_sample does, so no
// stream position moves and any thread computes any sample on its own; there is no rejection loop.  Box-Muller, one output per
// window:
//   U   = w[0] 2^64 + w[1]; e = its leading zero bits (U = 0: e = 127, U = 1); f in [1, 2) = the leading one of U << e and the
//         52 bits after it, truncated; u1 = f 2^(-e-1) in [2^-128, 1)
//   r   = sqrt(-2 ln u1) = sqrt(-2 (ln f - (e + 1) ln 2))             (at most sqrt(2 128 ln 2) = 13.32)
//   t   = w[2] >> 11 (53 bits), theta = 2 pi t / 2^53; z = r cos theta
//   result = rint(sigma z), ties to even; w[3 .. 5] are not used
//
// Bit identity.  ln, sin and cos are the polynomials below, not libm's or ocml's (which do not agree to the last bit).  The code
// uses +, -, *, / and sqrt on doubles and nothing else: each is correctly rounded on x86-64 and on gfx950 without fast-math, and
// conversions between integers and doubles here are exact.  There is NO fused multiply-add in it, and none may appear: every
// function that computes on doubles is declared FBS_FP_FN and opens with FBS_FP_STRICT, which together switch contraction off for
// its body whatever the defaults are (hipcc's device default fuses across statements, clang's host default within one, g++ fuses
// under -mfma): `#pragma clang fp contract(off)` in the body under clang and hipcc, the function attribute
// optimize("fp-contract=off") under g++.  (An explicit -ffp-contract=fast on a clang command line overrides the pragma; every build
// of this project passes -ffp-contract=off on top: csrc/Makefile, tests/c.)
//
// Accuracy: ln u1 to about 2^-51 relative (no cancellation: u1 = m 2^k with m in [sqrt(1/2), sqrt 2), so that u1 near 1 has k = 0
// and ln u1 = ln m is small AND accurate), sin and cos on [0, pi/4] to about 2^-52 relative, the octant reduction exact in
// integers: z to well below 2^-46 relative.  Not constant-time (branches on the octant and on f).
#pragma once
#include <stdint.h>

#include "fbs_chacha.hpp"

#if defined(__clang__)
#define FBS_FP_FN
#define FBS_FP_STRICT _Pragma("clang fp contract(off)")
#else
#define FBS_FP_FN __attribute__((optimize("fp-contract=off")))
#define FBS_FP_STRICT
#endif

namespace fbs {

constexpr uint32_t SAMPLER_IRWIN_HALL = 0, SAMPLER_GAUSS = 1;

// p v + c, as two roundings
FBS_FP_FN FBS_HD double gauss_step(double p, double v, double c) {
    FBS_FP_STRICT
    const double t = p * v;
    return t + c;
}

// -ln u1 for u1 = f 2^(-e-1), f in [1, 2), 0 <= e <= 127: positive, at most 128 ln 2
FBS_FP_FN FBS_HD double gauss_neg_log(double f, int e) {
    FBS_FP_STRICT
    // u1 = m 2^k, m in [sqrt(1/2), sqrt 2): k <= 0, and k = 0 only for u1 >= sqrt(1/2)
    int k = -e - 1;
    double m = f;
    if (f > 0x1.6a09e667f3bcdp+0) {   // sqrt 2
        m = f * 0.5;
        k += 1;
    }
    // ln m = 2 atanh(s), s = (m - 1) / (m + 1), |s| <= 0.1716: 2 s (1 + s^2 / 3 + s^4 / 5 + .. + s^20 / 21), next term 2^-60
    const double a = m - 1.0;         // (exact)
    const double b = m + 1.0;
    const double s = a / b;
    const double v = s * s;
    double p = 1.0 / 21.0;
    p = gauss_step(p, v, 1.0 / 19.0);
    p = gauss_step(p, v, 1.0 / 17.0);
    p = gauss_step(p, v, 1.0 / 15.0);
    p = gauss_step(p, v, 1.0 / 13.0);
    p = gauss_step(p, v, 1.0 / 11.0);
    p = gauss_step(p, v, 1.0 / 9.0);
    p = gauss_step(p, v, 1.0 / 7.0);
    p = gauss_step(p, v, 1.0 / 5.0);
    p = gauss_step(p, v, 1.0 / 3.0);
    const double sv = s * v;
    const double tail = sv * p;       // atanh(s) - s
    const double half_ln_m = s + tail;
    const double ln_m = half_ln_m + half_ln_m;
    // -k ln 2 in two parts: the high part has 32 trailing zero bits, so its product with -k <= 128 is exact
    const double nk = (double)(-k);
    const double hi = nk * 0x1.62e42feep-1;
    const double lo = nk * 0x1.a39ef35793c76p-33;
    const double rest = lo - ln_m;
    return hi + rest;
}

// cos(2 pi t / 2^53) for t < 2^53: the octant from the top three bits, the fraction of the octant (or its complement, in odd
// octants) exact in a double before its one multiplication by pi / 4, then sin or cos on [0, pi / 4]
FBS_FP_FN FBS_HD double gauss_cos_turn(uint64_t t) {
    FBS_FP_STRICT
    const uint32_t oct = (uint32_t)(t >> 50) & 7u;
    uint64_t g = t & ((1ull << 50) - 1);
    if (oct & 1u) g = (1ull << 50) - g;
    const double x = (double)(int64_t)g * 0x1p-50;   // (exact; the signed conversion is one instruction on both sides)
    const double y = x * 0x1.921fb54442d18p-1;       // pi / 4
    const double v = y * y;
    double c;
    if (((oct + 1u) >> 1) & 1u) {
        // octants 1, 2, 5, 6: sin y = y (1 - v/3! + v^2/5! - .. + v^8/17!), next term 2^-63
        double p = 1.0 / 355687428096000.0;
        p = gauss_step(p, v, -1.0 / 1307674368000.0);
        p = gauss_step(p, v, 1.0 / 6227020800.0);
        p = gauss_step(p, v, -1.0 / 39916800.0);
        p = gauss_step(p, v, 1.0 / 362880.0);
        p = gauss_step(p, v, -1.0 / 5040.0);
        p = gauss_step(p, v, 1.0 / 120.0);
        p = gauss_step(p, v, -1.0 / 6.0);
        const double yv = y * v;
        const double tail = yv * p;
        c = y + tail;
    } else {
        // octants 0, 3, 4, 7: cos y = 1 - v/2! + v^2/4! - .. - v^9/18!, next term 2^-68
        double p = -1.0 / 6402373705728000.0;
        p = gauss_step(p, v, 1.0 / 20922789888000.0);
        p = gauss_step(p, v, -1.0 / 87178291200.0);
        p = gauss_step(p, v, 1.0 / 479001600.0);
        p = gauss_step(p, v, -1.0 / 3628800.0);
        p = gauss_step(p, v, 1.0 / 40320.0);
        p = gauss_step(p, v, -1.0 / 720.0);
        p = gauss_step(p, v, 1.0 / 24.0);
        p = gauss_step(p, v, -0.5);
        c = gauss_step(p, v, 1.0);
    }
    return (((oct + 2u) >> 2) & 1u) ? -c : c;        // octants 2 .. 5: the left half of the circle
}

// the standard normal z of a window, before scaling: |z| <= 13.32
FBS_FP_FN FBS_HD double gauss_unit(const uint64_t w[6]) {
    FBS_FP_STRICT
    uint64_t top;   // the leading 64 bits of U << e
    int e;
    if (w[0]) {
        e = __builtin_clzll(w[0]);
        top = e ? (w[0] << e) | (w[1] >> (64 - e)) : w[0];
    } else if (w[1]) {
        const int z = __builtin_clzll(w[1]);
        e = 64 + z;
        top = w[1] << z;
    } else {
        e = 127;
        top = 1ull << 63;
    }
    const double f = (double)(int64_t)(top >> 11) * 0x1p-52;   // 53 bits: exact
    const double l = gauss_neg_log(f, e);
    const double r = __builtin_sqrt(l + l);
    const double c = gauss_cos_turn(w[2] >> 11);
    return r * c;
}

// sigma <= q < 2^46, so sigma z fits an int64 with room to spare; no draw when sigma is 0
FBS_FP_FN FBS_HD int64_t gauss_sample(const uint64_t w[6], uint64_t sigma) {
    FBS_FP_STRICT
    if (!sigma) return 0;
    const double v = (double)(int64_t)sigma * gauss_unit(w);
    return (int64_t)__builtin_rint(v);   // ties to even (the default rounding mode on the host, v_rndne_f64 on the device)
}

// the context's sampler applied to a window (fbs_params.sampler, checked at context creation)
FBS_HD int64_t sample_window(uint32_t sampler, const uint64_t w[6], uint64_t sigma) {
    return sampler == SAMPLER_GAUSS ? gauss_sample(w, sigma) : irwin_hall_sample(w, sigma);
}

}  // namespace fbs

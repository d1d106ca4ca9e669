// Packed outputs (include/fbs_exec.h, "packed outputs"): the arithmetic that the host and the device share.
//
// Up to N small-key ciphertexts at 31 bits a field (what fbs_compact_dev(bits = 31) packs) are written into the N coefficients of
// one GLWE sample under the big key by a packing key switch; the sample is rounded to w bits a coefficient and bit-packed like a
// compact ciphertext: k N mask fields (component-major), then the body fields of the coefficients in use.
#pragma once
#ifndef FBS_HOST_ONLY   // (the client library, libfbsclient.so, is built without HIP)
#include <hip/hip_runtime.h>
#endif

#include <cstddef>
#include <cstdint>

#include "fbs_compact.hpp"
#include "fbs_field.hpp"
#include "fbs_select.hpp"

namespace fbs {

static_assert(FQ == (1ull << 46) - 507903, "pack_lift_body is written for this q");

// null, or what (t, gamma) lacks to be a gadget key's parameters (a packing key's, a fold key's): 1 <= gamma, 1 <= t, t gamma <= 31;
// '#' stands for the letter of the key's parameters (check_gadget_params, fbs_api_checks.hpp)
inline const char *gadget_params_refused(uint32_t t, uint32_t gamma) {
    if (t < 1 || gamma < 1) return "t_# >= 1 and gamma_# >= 1";
    if (t > 31 || gamma > 31 || t * gamma > 31) return "t_# * gamma_# <= 31";
    return nullptr;
}

// is there a packing kernel for GLWE dimension k at N = 2^log_n?  (every shape a context can be created with: fbs_pack.hip)
inline bool pack_shape_built(uint32_t log_n, uint32_t k) { return k == 1 ? (log_n >= 8 && log_n <= 12) : glwe_shape_built(log_n, k); }

// h_v = round(q / 2^(gamma (v + 1))), gamma (v + 1) <= 31
FBS_HD uint64_t pack_gadget(uint32_t gamma, uint32_t v) {
    const uint64_t d = 1ull << (gamma * (v + 1));
    return (FQ + d / 2) / d;
}

// words of one packed sample that holds `fill` outputs (k N w is a multiple of 64: N >= 256), and of a batch of `count` outputs
FBS_HD size_t packed_sample_words(uint32_t k, uint32_t N, uint32_t fill, uint32_t bits) {
    return (size_t)k * N * bits / 64 + (size_t)(((uint64_t)fill * bits + 63) / 64);
}
FBS_HD size_t packed_words(uint32_t k, uint32_t N, size_t count, uint32_t bits) {
    const size_t full = count / N;
    const uint32_t rest = (uint32_t)(count % N);
    return full * packed_sample_words(k, N, N, bits) + (rest ? packed_sample_words(k, N, rest, bits) : 0);
}

// a mask field m < 2^31 rounded to tg = t_p gamma_p bits: ((m >> (r - 1)) + 1) >> 1 mod 2^tg with r = 31 - tg; m itself at r = 0
FBS_HD uint32_t pack_round_mask(uint32_t m, uint32_t tg) {
    const uint32_t r = 31 - tg;
    return r ? (((m >> (r - 1)) + 1) >> 1) & ((1u << tg) - 1u) : m;
}
// B/2 at every digit position: a' + offs cut into gamma-bit fields gives u_v = d_v + B/2 with d_v the BALANCED digits of a'
// (d_v in [-B/2, B/2), carries upwards, the carry out of the top dropped) -- the key switch's convention (fbs_kernels.hip)
FBS_HD uint32_t pack_digit_offsets(uint32_t t, uint32_t gamma) {
    uint32_t offs = 0;
    for (uint32_t v = 0; v < t; v++) offs |= (1u << (gamma - 1)) << (gamma * v);
    return offs;
}
// digit v (0 = most significant) of z = (a' + offs) mod 2^(t gamma)
FBS_HD int32_t pack_digit(uint32_t z, uint32_t v, uint32_t t, uint32_t gamma) {
    const uint32_t u = (z >> (gamma * (t - 1 - v))) & (uint32_t)((1ull << gamma) - 1);
    return (int32_t)u - (int32_t)(1u << (gamma - 1));
}
// the body field m < 2^31 lifted to Z_q: (m q + 2^30) >> 31 = m 2^15 + floor((2^30 - 507903 m) / 2^31), an exact integer below q
FBS_HD uint64_t pack_lift_body(uint32_t m) {
    return ((uint64_t)m << 15) + (uint64_t)(((int64_t)(1ll << 30) - (int64_t)m * 507903) >> 31);
}


#ifndef FBS_HOST_ONLY
// what the accumulate kernel reads (fbs_pack.hip), shared with the fold (fbs_fold.hip), whose rows are the D words of the big key
struct PackArgs {
    const uint32_t *fields;   // [n + 1][cols]: rounded mask fields, then the raw body fields (folding: [n][cols], then 64-bit bodies)
    const double *key;        // [n][t][k + 1][N]
    double *acc;              // [samples][slices][k + 1][N]
    const double *tw_fwd, *tw_inv;
    uint64_t *words;          // packed output of the launch (folding: the samples [k + 1][N])
    size_t count;             // ciphertexts of the launch
    size_t sample_words;      // words of a full sample
    uint32_t n, t, gamma, cols, slices, bits;
};
#endif

}  // namespace fbs

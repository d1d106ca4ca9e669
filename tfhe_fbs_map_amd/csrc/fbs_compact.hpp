// Compact output ciphertexts (include/fbs_exec.h, "compact outputs"): the arithmetic that the host and the device share.
//
// A compact ciphertext at width w is the big-key ciphertext key-switched to the small key and rounded to Z_(2^w) the way the
// modulus switch rounds to Z_2N (ms_store / k_ms_body, fbs_kernels.hip, with q treated as 2^46): n + 1 fields of w bits, mask
// first and body last, packed into W = ceil((n + 1) w / 64) words; field j occupies bits [j w, j w + w) of the ciphertext's bit
// stream, stream bit b being bit b mod 64 of word b / 64.
#pragma once
#ifndef FBS_HOST_ONLY   // (the client library, libfbsclient.so, is built without HIP)
#include <hip/hip_runtime.h>
#endif

#include <cstdint>

#include "fbs_field.hpp"

namespace fbs {

// words of one compact ciphertext of n + 1 fields of `bits` bits
FBS_HD uint32_t compact_words(uint32_t n, uint32_t bits) { return (uint32_t)(((uint64_t)(n + 1) * bits + 63) / 64); }

// the rounding of ms_store at modulus 2^bits: x in [0, 2^46) -> round(x 2^bits / 2^46) mod 2^bits
FBS_HD uint32_t compact_round(uint64_t x, uint32_t bits) {
    const uint32_t sh = FQ_BITS - bits;
    return (uint32_t)(((x >> (sh - 1)) + 1) >> 1) & ((1u << bits) - 1u);
}

// the modulus switch from 2^w down to 2^b (sh = w - b >= 1): a mask field x < 2^w -> round(x / 2^sh), not yet reduced mod 2^b
FBS_HD uint32_t compact_reround(uint32_t x, uint32_t sh) { return ((x >> (sh - 1)) + 1) >> 1; }
// the body of that switch: body' = (x_n - floor(eps / 2)) mod 2^w with eps the sum of the mask fields' signed errors
// x_i - (round(x_i / 2^sh) << sh), then rounded like a mask field (reduce mod 2^b after)
FBS_HD uint32_t compact_reround_body(uint32_t body, int64_t eps, uint32_t bits, uint32_t sh) {
    const uint32_t b2 = (uint32_t)((int64_t)body - (eps >> 1)) & ((1u << bits) - 1u);   // (>> floors)
    return compact_reround(b2, sh);
}

// field i of a packed ciphertext (fields never straddle more than two words: bits <= 31)
FBS_HD uint32_t compact_field(const uint64_t *ct, uint32_t i, uint32_t bits) {
    const uint64_t b = (uint64_t)i * bits;
    const uint32_t w = (uint32_t)(b >> 6), o = (uint32_t)(b & 63);
    uint64_t v = ct[w] >> o;
    if (o + bits > 64) v |= ct[w + 1] << (64 - o);
    return (uint32_t)v & ((1u << bits) - 1u);
}

// word j of a packed ciphertext from its fields: `field(f)` returns field f < n1 (already below 2^bits)
template <class Field>
FBS_HD uint64_t compact_word(uint32_t j, uint32_t n1, uint32_t bits, Field field) {
    const uint64_t b0 = (uint64_t)j * 64;
    uint64_t word = 0;
    for (uint32_t f = (uint32_t)(b0 / bits); f < n1 && (uint64_t)f * bits < b0 + 64; f++) {
        const uint64_t v = field(f);
        const int64_t sh = (int64_t)((uint64_t)f * bits) - (int64_t)b0;
        word |= sh >= 0 ? v << sh : v >> -sh;
    }
    return word;
}

// msg = round(phase 2p / 2^bits) mod 2p, phase = (body - sum_i m_i s_i) mod 2^bits; `sum` may be taken mod 2^32
FBS_HD int64_t compact_decode(uint32_t body, uint32_t sum, uint32_t bits, uint64_t two_p) {
    const uint64_t phase = (uint32_t)(body - sum) & ((1u << bits) - 1u);
    return (int64_t)(((phase * two_p + (1ull << (bits - 1))) >> bits) % two_p);   // phase 2p < 2^31 2^13
}

}  // namespace fbs

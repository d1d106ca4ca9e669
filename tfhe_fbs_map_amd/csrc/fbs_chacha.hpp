// ChaCha20 block function and the Irwin-Hall noise sample, shared by the host (rand_words / noise_sample, fbs_host.cpp) and the
// device encryption kernels (fbs_io.hip): both run this code, so a ciphertext made on either side is the same words.
// Original 64-bit-counter layout: key = the context's 8 words, words 12-13 the block counter, words 14-15 the stream id.
// Plain C++ as well (the HIP header only under hipcc): the sanitizer harness of tests/c builds fbs_host.cpp with g++.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

#include "fbs_field.hpp"

namespace fbs {

FBS_HD uint32_t chacha_rol(uint32_t v, int s) { return (v << s) | (v >> (32 - s)); }   // one v_alignbit_b32 on gfx950

FBS_HD void chacha_quarter(uint32_t &a, uint32_t &b, uint32_t &c, uint32_t &d) {
    a += b; d = chacha_rol(d ^ a, 16);
    c += d; b = chacha_rol(b ^ c, 12);
    a += b; d = chacha_rol(d ^ a, 8);
    c += d; b = chacha_rol(b ^ c, 7);
}

// block `counter` of stream `stream` under `key`: 64 bytes as 8 little-endian 64-bit words
FBS_HD void chacha_block(const uint32_t key[8], uint64_t stream, uint64_t counter, uint64_t out[8]) {
    uint32_t in[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u,
                       key[0], key[1], key[2], key[3], key[4], key[5], key[6], key[7],
                       (uint32_t)counter, (uint32_t)(counter >> 32), (uint32_t)stream, (uint32_t)(stream >> 32)};
    uint32_t x[16];
    for (int i = 0; i < 16; i++) x[i] = in[i];
    for (int round = 0; round < 20; round += 2) {
        chacha_quarter(x[0], x[4], x[8], x[12]); chacha_quarter(x[1], x[5], x[9], x[13]);
        chacha_quarter(x[2], x[6], x[10], x[14]); chacha_quarter(x[3], x[7], x[11], x[15]);
        chacha_quarter(x[0], x[5], x[10], x[15]); chacha_quarter(x[1], x[6], x[11], x[12]);
        chacha_quarter(x[2], x[7], x[8], x[13]); chacha_quarter(x[3], x[4], x[9], x[14]);
    }
    for (int i = 0; i < 8; i++) out[i] = (uint64_t)(x[2 * i] + in[2 * i]) | ((uint64_t)(x[2 * i + 1] + in[2 * i + 1]) << 32);
}

// Integer-only Gaussian stand-in from 6 random 64-bit words (Irwin-Hall, 12 uniform 32-bit terms, variance 2^64), scaled by
// sigma / 2^32 and rounded half-up.  Bounded at 6 sigma; fine for tests, not a production sampler.
FBS_HD int64_t irwin_hall_sample(const uint64_t w[6], uint64_t sigma) {
    __int128 s = -(__int128)6 * 0xFFFFFFFFll;
    for (int i = 0; i < 6; i++) s += (__int128)(uint32_t)w[i] + (__int128)(w[i] >> 32);
    return (int64_t)((s * (__int128)sigma + ((__int128)1 << 31)) >> 32);
}

}  // namespace fbs

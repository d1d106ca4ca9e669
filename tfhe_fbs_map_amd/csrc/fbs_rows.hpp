// The frame of an LWE row on the device: what k_encrypt, k_encrypt_seeded, k_expand_seeded (fbs_io.hip) and k_lwe_key_rows
// (fbs_keygen.hip) share, word for word what mask_words and lwe_body (fbs_host.cpp) compute.  A row is `len` folded words of a
// ChaCha20 stream (the mask) and a body = noise sample 0 of a second stream + <mask, secret bits> + a message.  One wave per row:
// a lane makes whole 64-byte blocks of the mask (8 words), consecutive lanes on consecutive blocks, and keeps its key-selected
// words in a 64-bit sum (len folded words stay below len 2^46 <= 2^58) that the wave adds up and reduces once.  Addressing, grids
// and the message term are each kernel's own.  Device code only: included by .hip files.
#pragma once
#include <hip/hip_runtime.h>

#include "fbs_chacha.hpp"
#include "fbs_internal.hpp"
#include "fbs_sampler.hpp"

namespace fbs {

typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));

// the sum of x over the 64 lanes of a wave, in every lane (integers: wrapping adds, any order gives the same words)
template <class T>
__device__ __forceinline__ T wave_sum(T x) {
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d);
    return x;
}

// words w[0 .. min(live, 8) - 1] of a block to p (8-byte aligned), by 16-byte stores where the block is whole.  Rows of an odd
// number of words (len + 1, len even) start on an odd word every other row, and so do all of a row's blocks: the branch is
// wave-uniform.  live < 8: the last block of a row whose length is no multiple of 8.
__device__ __forceinline__ void store_block(uint64_t *p, const uint64_t (&w)[8], uint32_t live) {
    if (live < 8) {
        for (uint32_t i = 0; i < live; i++) p[i] = w[i];
    } else if (((uintptr_t)p & 15u) == 0) {
        for (int i = 0; i < 8; i += 2) *reinterpret_cast<u64x2 *>(p + i) = u64x2{w[i], w[i + 1]};
    } else {
        p[0] = w[0];
        for (int i = 1; i < 7; i += 2) *reinterpret_cast<u64x2 *>(p + i) = u64x2{w[i], w[i + 1]};
        p[7] = w[7];
    }
}

// A lane's share of the mask of one row: blocks lane, lane + 64, .. of (key, stream), folded.  STORE: they go to row[0 .. len).
// sk_bits (packed, zero past len) non-null: returns the lane's part of sum_{s_i = 1} mask_i, not reduced; null: 0.
template <bool STORE>
__device__ __forceinline__ uint64_t lwe_mask_row(const RandKey &key, uint64_t stream, uint32_t len, uint64_t *row,
                                                 const uint32_t *sk_bits, uint32_t lane) {
    uint64_t sum = 0;
    for (uint32_t b = lane; b < (len + 7) / 8; b += 64) {
        uint64_t w[8];
        chacha_block(key.w, stream, b, w);   // mask words 8b .. 8b + 7
        const uint32_t bits = sk_bits ? (sk_bits[b >> 2] >> (8 * (b & 3))) & 0xFFu : 0u;
        for (int i = 0; i < 8; i++) {
            w[i] = fq_fold(w[i]);
            sum += ((bits >> i) & 1u) ? w[i] : 0;
        }
        if constexpr (STORE) store_block(row + 8 * (size_t)b, w, len - 8 * b);
    }
    return sum;
}

// the noise of a row's body as a residue: noise_sample(key, stream, idx 0, ..), words 0 .. 5 of block 0; no draw when sigma is 0
__device__ __forceinline__ uint64_t lwe_noise(const RandKey &key, uint64_t stream, uint32_t sampler, uint64_t sigma) {
    if (!sigma) return 0;
    uint64_t w[8];
    chacha_block(key.w, stream, 0, w);
    return fq_from_i64(sample_window(sampler, w, sigma));
}

}  // namespace fbs

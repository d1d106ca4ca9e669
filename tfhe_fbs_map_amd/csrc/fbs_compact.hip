// Compact output ciphertexts (include/fbs_exec.h, "compact outputs"), gfx950:
//
//   k_compact_pack      the fields the key switch left in the modulus-switched scratch, [count][n + 1] uint32 of `bits` bits
//                       each, -> [count][W] packed words (fbs_compact.hpp).  One workgroup per ciphertext: the fields a round of
//                       256 words spans are staged in LDS (coalesced 4-byte loads), then every lane assembles one word from
//                       the at most eight fields it overlaps and stores it (coalesced 8-byte stores).  Memory-bound: about
//                       3 KB in and 1 KB out per ciphertext.
//   k_decrypt_compact   the decode under the small key, what host_decrypt_compact returns: one wave per ciphertext, lanes
//                       striding over the mask fields, a 32-bit sum of the fields whose key bit is set (exact mod 2^w), the
//                       wave's sum, then round(phase 2p / 2^w) mod 2p.
//   k_compact_unpack    the way back, [count][W] packed words at width w -> the fields at b = log2(2N) bits in the modulus-switched
//                       scratch [count][n + 1], the rows the blind rotation reads (fbs_refresh_compact_dev, fbs_eval_sources).
//                       One wave per ciphertext, lanes striding over the fields (each spans at most two words, read through the
//                       cache: neighbouring lanes read neighbouring words), coalesced 4-byte stores.  At w = b a pure unpack; at
//                       w > b the mask fields are rounded to b bits as the modulus switch rounds (2^w in place of 2^46), their
//                       signed errors summed in 64 bits over the wave, and the body is taken down by floor(eps / 2) mod 2^w
//                       before its own rounding (compact_rerounded, fbs_compact.hpp).
//
// None is a key-switch or blind-rotation launch: they are not in fbs_kernel_catalog and the profile does not count them.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fbs_compact.hpp"
#include "fbs_rows.hpp"

namespace fbs {

constexpr uint32_t PACK_THREADS = 256;                          // words per round of k_compact_pack
constexpr uint32_t PACK_FIELDS = PACK_THREADS * 64 / 9 + 3;     // fields a round spans at the narrowest width (2N = 512: 9 bits)
constexpr size_t PACK_MAX_BLOCKS = 1u << 22;                    // workgroups per launch (2^22 x 256 work-items < 2^32)
constexpr uint32_t DEC_WAVES = 4;
constexpr uint32_t DEC_MAX_BLOCKS = 1u << 16;
constexpr uint32_t UNPACK_WAVES = 4;
constexpr uint32_t UNPACK_MAX_BLOCKS = 1u << 16;

__global__ __launch_bounds__(PACK_THREADS) void k_compact_pack(const uint32_t *ms, uint32_t n1, uint32_t bits, uint32_t W,
                                                               uint64_t *out) {
    __shared__ uint32_t fields[PACK_FIELDS];
    const uint32_t *row = ms + (size_t)blockIdx.x * n1;
    uint64_t *dst = out + (size_t)blockIdx.x * W;
    for (uint32_t w0 = 0; w0 < W; w0 += PACK_THREADS) {
        // fields [f0, f1) overlap words [w0, w0 + PACK_THREADS)
        const uint32_t f0 = (uint32_t)((uint64_t)w0 * 64 / bits);
        const uint32_t f1 = (uint32_t)std::min<uint64_t>(n1, ((uint64_t)(w0 + PACK_THREADS) * 64 + bits - 1) / bits);
        __syncthreads();   // (the previous round has read its fields)
        for (uint32_t f = f0 + threadIdx.x; f < f1; f += PACK_THREADS) fields[f - f0] = row[f];
        __syncthreads();
        const uint32_t j = w0 + threadIdx.x;
        if (j < W) dst[j] = compact_word(j, n1, bits, [&](uint32_t f) { return fields[f - f0]; });
    }
}

struct DecCompactArgs {
    const uint64_t *words;
    int64_t *msgs;
    size_t count;
    const uint32_t *sk;   // small LWE key, packed bits
    uint32_t n, bits, W;
    uint64_t two_p;
};

__global__ __launch_bounds__(64 * DEC_WAVES) void k_decrypt_compact(DecCompactArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    for (size_t c = (size_t)blockIdx.x * DEC_WAVES + threadIdx.x / 64; c < a.count; c += (size_t)gridDim.x * DEC_WAVES) {   // wave-uniform
        const uint64_t *ct = a.words + c * a.W;
        uint32_t sum = 0;   // mod 2^32, hence mod 2^bits
        for (uint32_t i = lane; i < a.n; i += 64)
            if ((a.sk[i >> 5] >> (i & 31u)) & 1u) sum += compact_field(ct, i, a.bits);
        sum = wave_sum(sum);
        if (lane == 0) a.msgs[c] = compact_decode(compact_field(ct, a.n, a.bits), sum, a.bits, a.two_p);
    }
}

struct UnpackArgs {
    const uint64_t *words;   // [count][W]
    uint32_t *ms;            // [count][n + 1]
    size_t count;
    uint32_t n, bits, W, b;  // b = log2(2N) <= bits
};

__global__ __launch_bounds__(64 * UNPACK_WAVES) void k_compact_unpack(UnpackArgs a) {
    const uint32_t lane = threadIdx.x & 63u, sh = a.bits - a.b, mask_b = (1u << a.b) - 1u;
    for (size_t c = (size_t)blockIdx.x * UNPACK_WAVES + threadIdx.x / 64; c < a.count; c += (size_t)gridDim.x * UNPACK_WAVES) {   // wave-uniform
        const uint64_t *ct = a.words + c * a.W;
        uint32_t *row = a.ms + c * (a.n + 1);
        if (sh == 0) {   // (uniform over the launch)
            for (uint32_t i = lane; i <= a.n; i += 64) row[i] = compact_field(ct, i, a.bits);
            continue;
        }
        int64_t eps = 0;
        for (uint32_t i = lane; i < a.n; i += 64) {
            const uint32_t x = compact_field(ct, i, a.bits), m = compact_reround(x, sh);
            eps += (int64_t)x - ((int64_t)m << sh);
            row[i] = m & mask_b;
        }
        eps = wave_sum(eps);
        if (lane == 0) row[a.n] = compact_reround_body(compact_field(ct, a.n, a.bits), eps, a.bits, sh) & mask_b;
    }
}

int dev_compact_unpack(const fbs_ctx *ctx, const uint64_t *d_words, size_t count, uint32_t bits, uint32_t *d_ms, hipStream_t stream) {
    if (count == 0) return FBS_OK;
    UnpackArgs a{};
    a.words = d_words;
    a.ms = d_ms;
    a.count = count;
    a.n = ctx->p.n;
    a.bits = bits;
    a.W = compact_words(ctx->p.n, bits);
    a.b = ctx->p.log_n_poly + 1;
    const dim3 grid((unsigned)std::min<size_t>((count + UNPACK_WAVES - 1) / UNPACK_WAVES, UNPACK_MAX_BLOCKS));
    hipLaunchKernelGGL(k_compact_unpack, grid, dim3(64 * UNPACK_WAVES), 0, stream, a);
    FBS_HIP(ctx, hipGetLastError());
    return FBS_OK;
}

int dev_compact_pack(const fbs_ctx *ctx, const uint32_t *d_ms, size_t count, uint32_t bits, uint64_t *d_words, hipStream_t stream) {
    const uint32_t n1 = ctx->p.n + 1, W = compact_words(ctx->p.n, bits);
    // one workgroup per ciphertext, and a grid dimension holds at most 2^32 work-items: launches of PACK_MAX_BLOCKS
    for (size_t c0 = 0; c0 < count; c0 += PACK_MAX_BLOCKS) {
        const size_t blocks = std::min<size_t>(PACK_MAX_BLOCKS, count - c0);
        hipLaunchKernelGGL(k_compact_pack, dim3((unsigned)blocks), dim3(PACK_THREADS), 0, stream, d_ms + c0 * n1, n1, bits, W, d_words + c0 * W);
        FBS_HIP(ctx, hipGetLastError());
    }
    return FBS_OK;
}

int dev_decrypt_compact(const fbs_ctx *ctx, const uint64_t *d_words, size_t count, uint32_t bits, int64_t *d_msgs, hipStream_t stream) {
    if (count == 0) return FBS_OK;
    DecCompactArgs a{};
    a.words = d_words;
    a.msgs = d_msgs;
    a.count = count;
    a.sk = ctx->d_sk_lwe_bits;
    a.n = ctx->p.n;
    a.bits = bits;
    a.W = compact_words(ctx->p.n, bits);
    a.two_p = 2ull * ctx->p.p_msg;
    const dim3 grid((unsigned)std::min<size_t>((count + DEC_WAVES - 1) / DEC_WAVES, DEC_MAX_BLOCKS));
    hipLaunchKernelGGL(k_decrypt_compact, grid, dim3(64 * DEC_WAVES), 0, stream, a);
    FBS_HIP(ctx, hipGetLastError());
    return FBS_OK;
}

}  // namespace fbs

// Encryption and decryption under the big key on the device (fbs_encrypt_dev, fbs_decrypt_dev, fbs_eval_messages), gfx950:
//
//   k_encrypt   word for word what host_encrypt (fbs_host.cpp) writes: the same ChaCha20 streams (fbs_chacha.hpp), the same
//               folds, the same body
//   k_decrypt   round(phase * 2p / q) mod 2p, what host_decrypt returns
//   k_encrypt_seeded   the body of host_encrypt_seeded: the mask of the seeded stream under the public mask key is summed, not
//               stored; noise and message under the context's key
//   k_debug_gauss      the rounded Gaussian alone on windows of words a test supplies (fbs_debug_gauss_dev)
//   k_expand_seeded    host_expand_seeded: the mask of the seeded stream under the mask key, then the given body.  No key-selected
//               sum: the kernel needs no secret, and is what an evaluation-only context runs on its inputs
//
// One wave per ciphertext, on the frame of fbs_rows.hpp (lwe_mask_row, lwe_noise); a kernel adds its addressing and its message.
// These kernels are not blind-rotation or key-switch launches: they are not in fbs_kernel_catalog and the profile does not count
// them.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fbs_rows.hpp"

namespace fbs {

constexpr uint32_t IO_WAVES = 4;              // waves (ciphertexts in flight) per workgroup
constexpr uint32_t IO_MAX_BLOCKS = 1u << 16;  // grid cap; the waves stride over the rest
constexpr uint32_t IO_NO_SLOT = 0xFFFFFFFFu;

struct EncArgs {
    IoView v;
    uint64_t nonce0, nonce_stride;   // ciphertext (r, s) takes stream nonce0 + r nonce_stride + s
    RandKey key;
    const uint32_t *sk;              // GLWE secret key, packed bits
    uint32_t D;
    uint64_t delta, sigma;
    uint32_t sampler;                // fbs_params.sampler: which noise sample (fbs_sampler.hpp); the same for every wave
};

struct DecArgs {
    IoView v;
    const uint32_t *sk;
    uint32_t D;
    uint64_t two_p;
};

__global__ __launch_bounds__(64 * IO_WAVES) void k_encrypt(EncArgs a) {
    const uint32_t lane = threadIdx.x & 63u, D = a.D;
    const size_t total = a.v.rows * a.v.per_row;
    for (size_t c = (size_t)blockIdx.x * IO_WAVES + threadIdx.x / 64; c < total; c += (size_t)gridDim.x * IO_WAVES) {   // wave-uniform
        const size_t r = c / a.v.per_row, s = c - r * a.v.per_row;
        const size_t slot = a.v.row_slot ? a.v.row_slot[r] : r;
        uint64_t *ct = a.v.cts + (slot * a.v.ct_stride + s) * (D + 1);
        const uint64_t nonce = a.nonce0 + r * a.nonce_stride + s;
        const uint64_t sum = wave_sum(lwe_mask_row<true>(a.key, stream_id(DOM_ENC_MASK, nonce), D, ct, a.sk, lane));
        if (lane == 63) {   // (the lane with the least mask work when the blocks do not fill the last round)
            const uint64_t body = fq_add(sum % FQ, lwe_noise(a.key, stream_id(DOM_ENC_NOISE, nonce), a.sampler, a.sigma));
            const int64_t m = a.v.msgs[r * a.v.msg_stride + s];
            ct[D] = fq_add(body, fq_mul(fq_from_i64(m), a.delta));
        }
    }
}

__global__ __launch_bounds__(64 * IO_WAVES) void k_decrypt(DecArgs a) {
    const uint32_t lane = threadIdx.x & 63u, D = a.D;
    const size_t total = a.v.rows * a.v.per_row;
    for (size_t c = (size_t)blockIdx.x * IO_WAVES + threadIdx.x / 64; c < total; c += (size_t)gridDim.x * IO_WAVES) {   // wave-uniform
        const size_t r = c / a.v.per_row, s = c - r * a.v.per_row;
        const uint32_t slot = a.v.row_slot ? a.v.row_slot[r] : (uint32_t)r;
        if (a.v.row_slot && slot == IO_NO_SLOT) continue;   // a constant output: the host fills it in
        const uint64_t *ct = a.v.cts + ((size_t)slot * a.v.ct_stride + s) * (D + 1);
        uint64_t sum = 0;
        for (uint32_t j = lane; j < D; j += 64) {
            const uint64_t w = ct[j];
            sum += ((a.sk[j >> 5] >> (j & 31u)) & 1u) ? w : 0;
        }
        sum = wave_sum(sum);
        if (lane == 0) {
            const uint64_t phase = fq_sub(ct[D], sum % FQ);
            const uint64_t v = phase * a.two_p + FQ / 2;   // < 2^46 * 2^13 + 2^45: no overflow
            a.v.msgs[r * a.v.msg_stride + s] = (int64_t)((v / FQ) % a.two_p);
        }
    }
}

struct SeededEncArgs {
    const int64_t *msgs;
    uint64_t *bodies;
    size_t count;
    uint64_t nonce0;                 // ciphertext i takes stream nonce0 + i
    RandKey mask_key, key;           // masks under the public mask key, noise under the context's key
    const uint32_t *sk;
    uint32_t D;
    uint64_t delta, sigma;
    uint32_t sampler;                // fbs_params.sampler: which noise sample (fbs_sampler.hpp); the same for every wave
};

struct ExpandArgs {
    IoView v;                        // v.msgs: the bodies, as uint64 words
    uint64_t nonce0, nonce_stride;   // ciphertext (r, s) takes stream nonce0 + r nonce_stride + s
    RandKey mask_key;
    uint32_t D;
};

__global__ __launch_bounds__(64 * IO_WAVES) void k_encrypt_seeded(SeededEncArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    for (size_t c = (size_t)blockIdx.x * IO_WAVES + threadIdx.x / 64; c < a.count; c += (size_t)gridDim.x * IO_WAVES) {   // wave-uniform
        const uint64_t nonce = a.nonce0 + c;
        const uint64_t sum = wave_sum(lwe_mask_row<false>(a.mask_key, stream_id(DOM_SENC_MASK, nonce), a.D, nullptr, a.sk, lane));
        if (lane == 63) {
            const uint64_t body = fq_add(sum % FQ, lwe_noise(a.key, stream_id(DOM_SENC_NOISE, nonce), a.sampler, a.sigma));
            a.bodies[c] = fq_add(body, fq_mul(fq_from_i64(a.msgs[c]), a.delta));
        }
    }
}

__global__ __launch_bounds__(64 * IO_WAVES) void k_expand_seeded(ExpandArgs a) {
    const uint32_t lane = threadIdx.x & 63u, D = a.D;
    const size_t total = a.v.rows * a.v.per_row;
    const uint64_t *bodies = reinterpret_cast<const uint64_t *>(a.v.msgs);
    for (size_t c = (size_t)blockIdx.x * IO_WAVES + threadIdx.x / 64; c < total; c += (size_t)gridDim.x * IO_WAVES) {   // wave-uniform
        const size_t r = c / a.v.per_row, s = c - r * a.v.per_row;
        const size_t slot = a.v.row_slot ? a.v.row_slot[r] : r;
        uint64_t *ct = a.v.cts + (slot * a.v.ct_stride + s) * (D + 1);
        lwe_mask_row<true>(a.mask_key, stream_id(DOM_SENC_MASK, a.nonce0 + r * a.nonce_stride + s), D, ct, nullptr, lane);
        if (lane == 63) ct[D] = bodies[r * a.v.msg_stride + s];
    }
}

static dim3 io_grid(size_t total) { return dim3((unsigned)std::min<size_t>((total + IO_WAVES - 1) / IO_WAVES, IO_MAX_BLOCKS)); }

int dev_upload_secret(fbs_ctx *ctx) {   // (both secret keys, as packed bits)
    const uint32_t D = ctx->D, words = (D + 31) / 32;
    std::vector<uint32_t> bits(words, 0);
    for (uint32_t j = 0; j < D; j++)
        if (ctx->sk_glwe[j]) bits[j >> 5] |= 1u << (j & 31);
    if (!ctx->d_sk_bits) FBS_HIP(ctx, hipMalloc(&ctx->d_sk_bits, (size_t)words * 4));
    FBS_HIP(ctx, hipMemcpy(ctx->d_sk_bits, bits.data(), (size_t)words * 4, hipMemcpyHostToDevice));
    // the small LWE key too: what compact outputs are decrypted under (fbs_decrypt_compact_dev)
    const uint32_t n = ctx->p.n, small_words = std::max(1u, (n + 31) / 32);
    std::vector<uint32_t> small(small_words, 0);
    for (uint32_t i = 0; i < n; i++)
        if (ctx->sk_lwe[i]) small[i >> 5] |= 1u << (i & 31);
    if (!ctx->d_sk_lwe_bits) FBS_HIP(ctx, hipMalloc(&ctx->d_sk_lwe_bits, (size_t)small_words * 4));
    FBS_HIP(ctx, hipMemcpy(ctx->d_sk_lwe_bits, small.data(), (size_t)small_words * 4, hipMemcpyHostToDevice));
    return FBS_OK;
}

int dev_encrypt(const fbs_ctx *ctx, const IoView &v, uint64_t nonce0, uint64_t nonce_stride, hipStream_t stream) {
    const size_t total = v.rows * v.per_row;
    if (total == 0) return FBS_OK;
    EncArgs a{};
    a.v = v;
    a.nonce0 = nonce0;
    a.nonce_stride = nonce_stride;
    a.key = ctx->rkey;
    a.sk = ctx->d_sk_bits;
    a.D = ctx->D;
    a.delta = 2 * ctx->delta_half;
    a.sigma = ctx->p.sigma_glwe;
    a.sampler = ctx->p.sampler;
    hipLaunchKernelGGL(k_encrypt, io_grid(total), dim3(64 * IO_WAVES), 0, stream, a);
    FBS_HIP(ctx, hipGetLastError());
    return FBS_OK;
}

int dev_decrypt(const fbs_ctx *ctx, const IoView &v, hipStream_t stream) {
    const size_t total = v.rows * v.per_row;
    if (total == 0) return FBS_OK;
    DecArgs a{};
    a.v = v;
    a.sk = ctx->d_sk_bits;
    a.D = ctx->D;
    a.two_p = 2ull * ctx->p.p_msg;
    hipLaunchKernelGGL(k_decrypt, io_grid(total), dim3(64 * IO_WAVES), 0, stream, a);
    FBS_HIP(ctx, hipGetLastError());
    return FBS_OK;
}

int dev_encrypt_seeded(const fbs_ctx *ctx, const int64_t *d_msgs, size_t count, uint64_t nonce0, uint64_t *d_bodies, hipStream_t stream) {
    if (count == 0) return FBS_OK;
    SeededEncArgs a{};
    a.msgs = d_msgs;
    a.bodies = d_bodies;
    a.count = count;
    a.nonce0 = nonce0;
    a.mask_key = ctx->mask_key;
    a.key = ctx->rkey;
    a.sk = ctx->d_sk_bits;
    a.D = ctx->D;
    a.delta = 2 * ctx->delta_half;
    a.sigma = ctx->p.sigma_glwe;
    a.sampler = ctx->p.sampler;
    hipLaunchKernelGGL(k_encrypt_seeded, io_grid(count), dim3(64 * IO_WAVES), 0, stream, a);
    FBS_HIP(ctx, hipGetLastError());
    return FBS_OK;
}

// test hook: the rounded Gaussian of `count` windows of six words, one thread each
__global__ __launch_bounds__(256) void k_debug_gauss(const uint64_t *words, size_t count, uint64_t sigma, int64_t *out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    uint64_t w[6];
    for (int j = 0; j < 6; j++) w[j] = words[6 * i + j];
    out[i] = gauss_sample(w, sigma);
}

int dev_debug_gauss(const fbs_ctx *ctx, const uint64_t *d_words, size_t count, uint64_t sigma, int64_t *d_out, hipStream_t stream) {
    if (count == 0) return FBS_OK;
    hipLaunchKernelGGL(k_debug_gauss, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream, d_words, count, sigma, d_out);
    FBS_HIP(ctx, hipGetLastError());
    return FBS_OK;
}

int dev_expand_seeded(const fbs_ctx *ctx, const IoView &v, uint64_t nonce0, uint64_t nonce_stride, hipStream_t stream) {
    const size_t total = v.rows * v.per_row;
    if (total == 0) return FBS_OK;
    ExpandArgs a{};
    a.v = v;
    a.nonce0 = nonce0;
    a.nonce_stride = nonce_stride;
    a.mask_key = ctx->mask_key;
    a.D = ctx->D;
    hipLaunchKernelGGL(k_expand_seeded, io_grid(total), dim3(64 * IO_WAVES), 0, stream, a);
    FBS_HIP(ctx, hipGetLastError());
    return FBS_OK;
}

}  // namespace fbs

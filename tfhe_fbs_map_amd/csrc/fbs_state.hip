// Resident state (fbs_state, fbs_eval_resident), gfx950: ciphertexts between the rows of state blocks [rows][T][D + 1] and the wire
// slots [n_slots][Tc][D + 1] of a chunk; and the plaintext inputs of a chunk (FBS_SRC_PLAIN), written into the same slots.
//
//   k_state_gather    wire slot of link e, sample q  <-  row of link e, sample s0 + q     (the resident inputs of a chunk)
//   k_state_scatter   row of link e, sample s0 + q   <-  wire slot of link e, sample q    (its outputs; a constant output is
//                     written as the trivial ciphertext fbs_eval returns for it)
//   k_fill_plain      wire slot of link e, sample q  <-  the trivial ciphertext of the link's message for sample q (the plaintext
//                     inputs of a chunk, FBS_SRC_PLAIN: D zero words, then m Delta mod q)
//
// One launch moves every link of the chunk: the (link, sample) grid is dealt to waves, one ciphertext per wave at a time.  A
// ciphertext is D + 1 words, an odd number, so one at an odd index starts 8 bytes off a 16-byte line.  Where source and
// destination agree in that, the wave moves 16 bytes a lane each way, with the one word before or after the pairs on its own
// (as k_expand_seeded stores its blocks); where they differ, the stores stay 16 bytes wide and aligned and each takes two 8-byte
// loads -- consecutive lanes on consecutive words either way.  Plain vector loads and stores only.  These kernels are copies: they
// are not in fbs_kernel_catalog and the profile does not count them.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fbs_internal.hpp"

namespace fbs {

constexpr uint32_t ST_WAVES = 4;              // waves (ciphertexts in flight) per workgroup
constexpr uint32_t ST_MAX_BLOCKS = 1u << 16;  // grid cap; the waves stride over the rest

typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));

// `words` words (odd: D + 1) from src to dst, both 8-byte aligned, by the 64 lanes of one wave
__device__ __forceinline__ void wave_copy_ct(uint64_t *dst, const uint64_t *src, uint32_t words, uint32_t lane) {
    const uint32_t head = (uint32_t)(((uintptr_t)dst >> 3) & 1u);   // words before dst's first 16-byte line
    const uint32_t pairs = (words - head) / 2;
    const bool src_aligned = (((uintptr_t)(src + head)) & 15u) == 0;   // wave-uniform
    if (src_aligned) {
        for (uint32_t j = lane; j < pairs; j += 64)
            *reinterpret_cast<u64x2 *>(dst + head + 2 * j) = *reinterpret_cast<const u64x2 *>(src + head + 2 * j);
    } else {
        for (uint32_t j = lane; j < pairs; j += 64) {
            const uint64_t *p = src + head + 2 * j;
            *reinterpret_cast<u64x2 *>(dst + head + 2 * j) = u64x2{p[0], p[1]};
        }
    }
    if (lane == 63) {   // the words the pairs leave: the first (head = 1) or the last (head = 0; words is odd)
        if (head) dst[0] = src[0];
        else dst[words - 1] = src[words - 1];
    }
}

// the trivial ciphertext (0, .., 0, body)
__device__ __forceinline__ void wave_fill_trivial(uint64_t *dst, uint64_t body, uint32_t words, uint32_t lane) {
    const uint32_t head = (uint32_t)(((uintptr_t)dst >> 3) & 1u);
    const uint32_t pairs = (words - head) / 2;
    for (uint32_t j = lane; j < pairs; j += 64) {
        const uint32_t w = head + 2 * j;
        *reinterpret_cast<u64x2 *>(dst + w) = u64x2{0, w + 1 == words - 1 ? body : 0};
    }
    if (lane == 63) {
        if (head) dst[0] = 0;
        else dst[words - 1] = body;
    }
}

__global__ __launch_bounds__(64 * ST_WAVES) void k_state_gather(StateCopy a) {
    const uint32_t lane = threadIdx.x & 63u, words = a.D + 1;
    const size_t total = a.n_links * a.tc;
    for (size_t c = (size_t)blockIdx.x * ST_WAVES + threadIdx.x / 64; c < total; c += (size_t)gridDim.x * ST_WAVES) {   // wave-uniform
        const size_t e = c / a.tc, q = c - e * a.tc;
        const StateLink ln = a.links[e];
        wave_copy_ct(a.wires + ((size_t)ln.slot * a.Tc + q) * words, ln.row + (a.s0 + q) * words, words, lane);
    }
}

__global__ __launch_bounds__(64 * ST_WAVES) void k_state_scatter(StateCopy a) {
    const uint32_t lane = threadIdx.x & 63u, words = a.D + 1;
    const size_t total = a.n_links * a.tc;
    for (size_t c = (size_t)blockIdx.x * ST_WAVES + threadIdx.x / 64; c < total; c += (size_t)gridDim.x * ST_WAVES) {   // wave-uniform
        const size_t e = c / a.tc, q = c - e * a.tc;
        const StateLink ln = a.links[e];
        uint64_t *dst = ln.row + (a.s0 + q) * words;
        if (ln.slot & STATE_LINK_CONST) wave_fill_trivial(dst, ln.slot & ~STATE_LINK_CONST, words, lane);
        else wave_copy_ct(dst, a.wires + ((size_t)ln.slot * a.Tc + q) * words, words, lane);
    }
}

// A pure streaming write: the wave stores 16 bytes a lane, aligned to the destination (wave_fill_trivial), and the body -- the only
// non-zero word -- is computed once per ciphertext, wave-uniform.  m < 2p (checked by the host) and Delta <= q / 2p + 1, so
// m Delta < q + 2p fits 64 bits and one 64-bit remainder is the residue fbs_eval's trivial_body computes.
__global__ __launch_bounds__(64 * ST_WAVES) void k_fill_plain(PlainFill a) {
    const uint32_t lane = threadIdx.x & 63u, words = a.D + 1;
    const size_t total = a.n_links * a.tc;
    for (size_t c = (size_t)blockIdx.x * ST_WAVES + threadIdx.x / 64; c < total; c += (size_t)gridDim.x * ST_WAVES) {   // wave-uniform
        const size_t e = c / a.tc, q = c - e * a.tc;
        const PlainLink ln = a.links[e];
        const uint64_t m = (uint64_t)(ln.msgs ? ln.msgs[q] : ln.value);
        wave_fill_trivial(a.wires + ((size_t)ln.slot * a.Tc + q) * words, m * a.delta % FQ, words, lane);
    }
}

static dim3 st_grid(size_t total) { return dim3((unsigned)std::min<size_t>((total + ST_WAVES - 1) / ST_WAVES, ST_MAX_BLOCKS)); }

int dev_state_gather(const fbs_ctx *ctx, const StateCopy &a, hipStream_t stream) {
    if (a.n_links * a.tc == 0) return FBS_OK;
    hipLaunchKernelGGL(k_state_gather, st_grid(a.n_links * a.tc), dim3(64 * ST_WAVES), 0, stream, a);
    FBS_HIP(ctx, hipGetLastError());
    return FBS_OK;
}

int dev_state_scatter(const fbs_ctx *ctx, const StateCopy &a, hipStream_t stream) {
    if (a.n_links * a.tc == 0) return FBS_OK;
    hipLaunchKernelGGL(k_state_scatter, st_grid(a.n_links * a.tc), dim3(64 * ST_WAVES), 0, stream, a);
    FBS_HIP(ctx, hipGetLastError());
    return FBS_OK;
}

int dev_fill_plain(const fbs_ctx *ctx, const PlainFill &a, hipStream_t stream) {
    if (a.n_links * a.tc == 0) return FBS_OK;
    hipLaunchKernelGGL(k_fill_plain, st_grid(a.n_links * a.tc), dim3(64 * ST_WAVES), 0, stream, a);
    FBS_HIP(ctx, hipGetLastError());
    return FBS_OK;
}

}  // namespace fbs

// Encrypted tables, gfx950 (include/fbs_exec.h, "encrypted tables"): what a write by an encrypted index needs beside the mapped fold
// and the blind rotation, which it uses as they stand.
//
//   k_ms_negate   every rotation amount a of the modulus-switched rows -> (2N - a) mod 2N.  A write adds X^{+r} U where a read takes
//                 X^{-r} of the table: the rotation kernels turn by -r, so the write hands them the negated amounts, masks and body
//                 alike.  Zero stays zero -- a skipped step stays skipped -- and at two key bits a step the kernels derive the
//                 bundle's third exponent from the negated pair themselves.
//   k_glwe_add    sample dst_of[f] of dst  +=  sample f of src, word by word modulo q, (k + 1) N words a sample.  The host has
//                 checked dst_of: in range, and no target twice, so no two lanes of a launch meet in one word.
//   k_ct_sub      ciphertext f of out  =  ciphertext a_of[f] of a  -  ciphertext f of b, word by word modulo q: the delta of a SET,
//                 value minus the refreshed old entry, which the add steps then write.  Without b it gathers an ADD's values into
//                 the tables' order, so that every write folds under the table object's one set of unit-box maps.
//
// The first two are streaming kernels of 16 bytes a lane, the third of 8 (a ciphertext has an odd number of words), with plain
// vector loads and stores; a grid-stride loop covers what the grid cap leaves.  They are not in fbs_kernel_catalog and the profile does not count them.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fbs_field.hpp"
#include "fbs_rows.hpp"

namespace fbs {

constexpr uint32_t TB_LANES = 256;
constexpr size_t TB_MAX_BLOCKS = 1u << 20;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// `quads` whole groups of four amounts, then the `words - 4 quads` < 4 that are left; ms is a device allocation (256-byte aligned)
__global__ __launch_bounds__(TB_LANES) void k_ms_negate(uint32_t *__restrict__ ms, size_t words, uint32_t mask) {
    const size_t quads = words / 4, step = (size_t)gridDim.x * TB_LANES, first = (size_t)blockIdx.x * TB_LANES + threadIdx.x;
    for (size_t i = first; i < quads; i += step) {
        u32x4 *p = reinterpret_cast<u32x4 *>(ms) + i;
        const u32x4 v = *p;
        *p = u32x4{(0u - v.x) & mask, (0u - v.y) & mask, (0u - v.z) & mask, (0u - v.w) & mask};
    }
    if (first < words - 4 * quads) ms[4 * quads + first] = (0u - ms[4 * quads + first]) & mask;
}

// pairs = (k + 1) N / 2 16-byte pairs a sample; total = count pairs
__global__ __launch_bounds__(TB_LANES) void k_glwe_add(uint64_t *__restrict__ dst, const uint64_t *__restrict__ src,
                                                       const uint32_t *__restrict__ dst_of, size_t pairs, size_t total) {
    const u64x2 *from = reinterpret_cast<const u64x2 *>(src);
    u64x2 *to = reinterpret_cast<u64x2 *>(dst);
    for (size_t i = (size_t)blockIdx.x * TB_LANES + threadIdx.x; i < total; i += (size_t)gridDim.x * TB_LANES) {
        const size_t f = i / pairs, j = i - f * pairs;
        u64x2 *p = to + (size_t)dst_of[f] * pairs + j;
        const u64x2 a = from[i], b = *p;
        *p = u64x2{fq_add(a.x, b.x), fq_add(a.y, b.y)};
    }
}

// ct_words = D + 1 is odd: a ciphertext at an odd index starts 8 bytes off a 16-byte line, so this one moves 8 bytes a lane,
// consecutive lanes on consecutive words
__global__ __launch_bounds__(TB_LANES) void k_ct_sub(const uint64_t *__restrict__ a, const uint32_t *__restrict__ a_of, const uint64_t *b,
                                                     uint64_t *out, size_t ct_words, size_t total) {
    for (size_t i = (size_t)blockIdx.x * TB_LANES + threadIdx.x; i < total; i += (size_t)gridDim.x * TB_LANES) {
        const size_t f = i / ct_words, w = i - f * ct_words;
        const uint64_t x = a[(size_t)a_of[f] * ct_words + w];
        out[i] = b ? fq_sub(x, b[i]) : x;   // (b null, kernel-uniform: a gather)
    }
}

static dim3 tb_grid(size_t items) { return dim3((unsigned)std::min((items + TB_LANES - 1) / TB_LANES, TB_MAX_BLOCKS)); }

int dev_ms_negate(const fbs_ctx *ctx, uint32_t *d_ms, size_t rows, hipStream_t stream) {
    const size_t words = rows * (ctx->p.n + 1);
    if (words == 0) return FBS_OK;
    hipLaunchKernelGGL(k_ms_negate, tb_grid(std::max<size_t>(words / 4, 4)), dim3(TB_LANES), 0, stream, d_ms, words, 2u * ctx->N - 1u);
    FBS_HIP(ctx, hipGetLastError());
    return FBS_OK;
}

int dev_glwe_add(const fbs_ctx *ctx, uint64_t *d_dst, const uint64_t *d_src, const uint32_t *d_dst_of, size_t count, hipStream_t stream) {
    const size_t pairs = (size_t)(ctx->p.k + 1) * ctx->N / 2;
    if (count == 0) return FBS_OK;
    hipLaunchKernelGGL(k_glwe_add, tb_grid(count * pairs), dim3(TB_LANES), 0, stream, d_dst, d_src, d_dst_of, pairs, count * pairs);
    FBS_HIP(ctx, hipGetLastError());
    return FBS_OK;
}

int dev_ct_sub(const fbs_ctx *ctx, const uint64_t *d_a, const uint32_t *d_a_of, const uint64_t *d_b, uint64_t *d_out, size_t count, hipStream_t stream) {
    const size_t ct_words = (size_t)ctx->D + 1;
    if (count == 0) return FBS_OK;
    hipLaunchKernelGGL(k_ct_sub, tb_grid(count * ct_words), dim3(TB_LANES), 0, stream, d_a, d_a_of, d_b, d_out, ct_words, count * ct_words);
    FBS_HIP(ctx, hipGetLastError());
    return FBS_OK;
}

}  // namespace fbs

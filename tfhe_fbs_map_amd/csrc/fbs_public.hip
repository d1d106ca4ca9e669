// Public-key inputs (include/fbs_exec.h, "public-key inputs"), gfx950: the server's side, sample extraction of GLWE samples
// [k + 1][N] into big-key ciphertexts [D + 1] -- data movement with a sign.
//
//   k_expand_public   ciphertext j  <-  coefficient t = j mod N of sample j / N:
//                     word c N + i = A'_c[t - i] (i <= t), q - A'_c[N + t - i] (i > t; zero stays zero), word D = B'[t]
//
// One sample feeds N ciphertexts, 8 (D + 1) N bytes written from 8 (k + 1) N read, and every ciphertext reads all k N mask words.
// A workgroup takes PX_ROWS consecutive coefficients of one sample: it reads the sample's masks from memory once into LDS (8 k N
// bytes: 16 KB at k = 2, N = 1024, 32 KB at k = 1, N = 4096), then each wave writes whole ciphertexts as wave_fill_trivial of
// fbs_state.hip does -- 16 bytes a lane, aligned to the DESTINATION (D + 1 is odd: every other ciphertext starts 8 bytes off a
// 16-byte line, and the one word the pairs leave goes on its own).  The source index runs backwards as the destination runs
// forwards: consecutive lanes read consecutive pairs of LDS words in reverse, and the negation and the wrap at i = t are computed
// on the way.  Plain vector loads and stores only.  Like the other copy kernels it is not in fbs_kernel_catalog.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fbs_rows.hpp"

namespace fbs {

constexpr uint32_t PX_WAVES = 4;              // waves per workgroup
constexpr uint32_t PX_ROWS = 16;              // coefficients (ciphertexts) of one sample per workgroup; divides every N
constexpr uint32_t PX_MAX_BLOCKS = 1u << 16;  // grid cap; the workgroups stride over the rest

struct PubExpand {
    const uint64_t *glwe;   // [ceil(count / N)][k + 1][N]
    uint64_t *cts;          // [count][D + 1]
    size_t count;
    uint32_t N, D;          // N a power of two, D = k N
};

__global__ __launch_bounds__(64 * PX_WAVES) void k_expand_public(PubExpand a) {
    extern __shared__ __attribute__((aligned(16))) uint64_t masks[];   // [k][N]
    const uint32_t N = a.N, D = a.D, words = D + 1, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t slices = N / PX_ROWS;
    const size_t items = ((a.count + N - 1) / N) * slices;
    for (size_t item = blockIdx.x; item < items; item += gridDim.x) {   // (sample, slice): uniform over the workgroup
        const size_t g = item / slices;
        const uint32_t t0 = (uint32_t)(item - g * slices) * PX_ROWS;
        if (g * N + t0 >= a.count) continue;   // past the fill of the last sample: never extracted
        const uint64_t *sample = a.glwe + g * ((size_t)D + N);
        __syncthreads();   // (the rows of the previous item have been read)
        for (uint32_t i = threadIdx.x; i < D; i += 64 * PX_WAVES) masks[i] = sample[i];
        __syncthreads();
        for (uint32_t t = t0 + wave; t < t0 + PX_ROWS && g * N + t < a.count; t += PX_WAVES) {   // wave-uniform
            uint64_t *dst = a.cts + (g * N + t) * words;
            const uint64_t body = sample[D + t];
            auto word = [&](uint32_t w) -> uint64_t {   // w < D
                const uint32_t i = w & (N - 1);
                const uint64_t x = masks[(w - i) + ((t - i) & (N - 1))];
                return (i > t && x) ? FQ - x : x;
            };
            const uint32_t head = (uint32_t)(((uintptr_t)dst >> 3) & 1u);   // words before dst's first 16-byte line
            const uint32_t pairs = (words - head) / 2;
            for (uint32_t j = lane; j < pairs; j += 64) {
                const uint32_t w = head + 2 * j;   // w + 1 <= D, and w + 1 == D only where head = 1
                const uint64_t lo = word(w);
                const uint64_t hi = w + 1 == D ? body : word(w + 1);
                *reinterpret_cast<u64x2 *>(dst + w) = u64x2{lo, hi};
            }
            if (lane == 63) {   // the word the pairs leave: the first (head = 1) or the last (head = 0)
                if (head) dst[0] = word(0);
                else dst[D] = body;
            }
        }
    }
}

int dev_expand_public(const fbs_ctx *ctx, const uint64_t *d_glwe, size_t count, uint64_t *d_cts, hipStream_t stream) {
    if (count == 0) return FBS_OK;
    PubExpand a{};
    a.glwe = d_glwe;
    a.cts = d_cts;
    a.count = count;
    a.N = ctx->N;
    a.D = ctx->D;
    static_assert(256 % PX_ROWS == 0 && PX_ROWS % PX_WAVES == 0, "a slice is whole rounds of the waves and divides the smallest N");
    const size_t items = ((count + ctx->N - 1) / ctx->N) * (ctx->N / PX_ROWS);
    hipLaunchKernelGGL(k_expand_public, dim3((unsigned)std::min<size_t>(items, PX_MAX_BLOCKS)), dim3(64 * PX_WAVES), (size_t)ctx->D * 8, stream, a);
    FBS_HIP(ctx, hipGetLastError());
    return FBS_OK;
}

}  // namespace fbs

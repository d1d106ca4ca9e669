// Folded state (include/fbs_exec.h, "folded state"), gfx950: up to N big-key ciphertexts into the N coefficients of one GLWE
// sample under the same key, at full precision -- a packing key switch taken straight from the big key, on the accumulate kernel of
// the packed outputs (fbs_pack.hip: no new arithmetic), between a front and a finish kernel of its own.
//
//   k_fold_front        the ciphertexts of a pass, [ciphertext][D + 1] 64-bit words, -> the mask words rounded to t_f gamma_f bits
//                       (compact_round: the key switch's own rounding, the integer function ks_round computes before its digit
//                       offsets), [D][samples N] uint32, then the raw body words [samples N] uint64.  64 ciphertexts x 128 words a
//                       workgroup through an LDS tile.  A wave reads one source row segment at a time, 16 bytes a lane, aligned
//                       to the SOURCE: D + 1 is odd, so every other row starts 8 bytes off a 16-byte line; the word the pairs
//                       leave at either end is read on its own (the cases of wave_copy_ct).  No lane reads with the stride of a
//                       ciphertext.  Stores are 256 coalesced bytes a wave.  Ciphertexts past `count` are not read: zero.
//   k_fold_front_mapped the same front for a MAPPED fold ("encrypted-index reads"): position j takes ciphertext map[j], negated or
//                       none at all as the map says; everything behind it is the fold's own.
//   k_pack_accumulate   (fbs_pack.hip, as it stands) with n := D, the fields above and the fold key: its slicing for launches of
//                       few samples, its common row order, PACK_CENTRE_EVERY.
//   k_fold_finish       one workgroup per (sample, component): the slices summed, inverse transform, negated, the raw body words
//                       added on component k, canonical residues written 16 bytes a lane from LDS.  No rounding, no bit packing.
//
// Every value is an exact residue: the words do not depend on slicing or launch shape (tests/test_gpu_fold.py, word for word
// against tests/fold_reference.py).  None of these is a key-switch or blind-rotation launch: they are not in fbs_kernel_catalog.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fbs_blind_rotate.hpp"
#include "fbs_pack.hpp"
#include "fbs_rows.hpp"

namespace fbs {

constexpr uint32_t FF_ROWS = 64;    // ciphertexts of a tile
constexpr uint32_t FF_COLS = 128;   // mask words of a tile: one 16-byte load a lane

// cts [count][D + 1] -> fields [D][cols] (rounded to tg bits), then bodies [cols] (64-bit, at fields + D cols); D a multiple of
// FF_COLS, cols a multiple of FF_ROWS; grid (D / FF_COLS, cols / FF_ROWS), 256 threads
__global__ __launch_bounds__(256) void k_fold_front(const uint64_t *__restrict__ cts, uint32_t D, size_t count, uint32_t cols, uint32_t tg,
                                                    uint32_t *__restrict__ fields) {
    __shared__ uint32_t tile[FF_ROWS][FF_COLS + 1];
    __shared__ uint64_t bodies[FF_ROWS];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t w0 = blockIdx.x * FF_COLS, j0 = blockIdx.y * FF_ROWS;
    const bool last = w0 + FF_COLS == D;                    // this tile also takes the body word, column D
    const uint32_t w1 = w0 + FF_COLS + (last ? 1u : 0u);    // words [w0, w1) of a row
    auto put = [&](uint32_t r, uint32_t w, uint64_t x) {    // w in [w0, w1)
        if (w == D) bodies[r] = x;
        else tile[r][w - w0] = compact_round(x, tg);
    };
#pragma unroll 4
    for (uint32_t r = wave; r < FF_ROWS; r += 4) {          // wave-uniform
        const size_t j = (size_t)j0 + r;
        if (j >= count) {
            tile[r][lane] = 0u;
            tile[r][lane + 64] = 0u;
            if (lane == 0) bodies[r] = 0;
            continue;
        }
        const uint64_t *row = cts + j * ((size_t)D + 1);
        const uint32_t head = (uint32_t)(((uintptr_t)(row + w0) >> 3) & 1u);   // words before the segment's first 16-byte line
        const uint32_t w = w0 + head + 2 * lane;
        if (w + 1 < w1) {
            const u64x2 p = *reinterpret_cast<const u64x2 *>(row + w);
            put(r, w, p[0]);
            put(r, w + 1, p[1]);
        } else if (w < w1) {
            put(r, w, row[w]);
        }
        if (lane == 63) {   // the word the pairs leave: the first (head = 1), or the body behind a whole run of pairs (head = 0)
            if (head) put(r, w0, row[w0]);
            else if (last) put(r, D, row[D]);
        }
    }
    __syncthreads();
    for (uint32_t c = wave; c < FF_COLS; c += 4) fields[(size_t)(w0 + c) * cols + j0 + lane] = tile[lane][c];
    if (last && threadIdx.x < FF_ROWS) reinterpret_cast<uint64_t *>(fields + (size_t)D * cols)[j0 + threadIdx.x] = bodies[threadIdx.x];
}

// The mapped fold's front ("encrypted-index reads" in include/fbs_exec.h): position j of the pass takes ciphertext map[j] of the
// n_src at cts instead of ciphertext j -- the same tile, the same source-aligned 16-byte row reads, the same stores.  Bit 31 of
// map[j]: every word of the ciphertext, masks and body, is negated (fq_neg) before anything else, so the rounding sees what it
// would see in the materialised array.  FOLD_MAP_NONE: no ciphertext, zero words, as past `count`.  The map is device memory the
// host cannot check: an index at or past n_src reads ciphertext 0, never past the array.  A box map names the same source N / p
// positions running, so most of a tile's rows re-read one row out of L2.
__global__ __launch_bounds__(256) void k_fold_front_mapped(const uint64_t *__restrict__ cts, size_t n_src, const uint32_t *__restrict__ map,
                                                           uint32_t D, size_t count, uint32_t cols, uint32_t tg, uint32_t *__restrict__ fields) {
    __shared__ uint32_t tile[FF_ROWS][FF_COLS + 1];
    __shared__ uint64_t bodies[FF_ROWS];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t w0 = blockIdx.x * FF_COLS, j0 = blockIdx.y * FF_ROWS;
    const bool last = w0 + FF_COLS == D;
    const uint32_t w1 = w0 + FF_COLS + (last ? 1u : 0u);
#pragma unroll 4
    for (uint32_t r = wave; r < FF_ROWS; r += 4) {          // wave-uniform
        const size_t j = (size_t)j0 + r;
        const uint32_t m = j < count ? map[j] : FOLD_MAP_NONE;
        if (m == FOLD_MAP_NONE) {
            tile[r][lane] = 0u;
            tile[r][lane + 64] = 0u;
            if (lane == 0) bodies[r] = 0;
            continue;
        }
        const bool neg = (m & 0x80000000u) != 0;
        size_t src = m & 0x7FFFFFFFu;
        if (src >= n_src) src = 0;
        auto put = [&](uint32_t w, uint64_t x) {            // w in [w0, w1)
            if (neg) x = fq_neg(x);
            if (w == D) bodies[r] = x;
            else tile[r][w - w0] = compact_round(x, tg);
        };
        const uint64_t *row = cts + src * ((size_t)D + 1);
        const uint32_t head = (uint32_t)(((uintptr_t)(row + w0) >> 3) & 1u);
        const uint32_t w = w0 + head + 2 * lane;
        if (w + 1 < w1) {
            const u64x2 p = *reinterpret_cast<const u64x2 *>(row + w);
            put(w, p[0]);
            put(w + 1, p[1]);
        } else if (w < w1) {
            put(w, row[w]);
        }
        if (lane == 63) {
            if (head) put(w0, row[w0]);
            else if (last) put(D, row[D]);
        }
    }
    __syncthreads();
    for (uint32_t c = wave; c < FF_COLS; c += 4) fields[(size_t)(w0 + c) * cols + j0 + lane] = tile[lane][c];
    if (last && threadIdx.x < FF_ROWS) reinterpret_cast<uint64_t *>(fields + (size_t)D * cols)[j0 + threadIdx.x] = bodies[threadIdx.x];
}

// grid: samples * (k + 1) workgroups, component fastest; a.words [samples][k + 1][N], 16-byte aligned
template <int LOGN, int LL>
__global__ __launch_bounds__(1 << LL) void k_fold_finish(PackArgs a, uint32_t k1) {
    using W = typename NttFor<LOGN, LL>::type;
    constexpr int N = W::N, E = W::E, LANES = W::LANES;
    __shared__ __attribute__((aligned(16))) double lds[2 * N];
    const uint32_t t = threadIdx.x;
    const uint32_t g = blockIdx.x / k1, c = blockIdx.x % k1;
    typename W::Xchg xc{lds, 0};
    double x[E];
#pragma unroll
    for (int m = 0; m < E; m++) x[m] = 0.0;
    for (uint32_t s = 0; s < a.slices; s++) {   // at most PACK_MAX_SLICES centred residues
        const double *src = a.acc + (((size_t)g * a.slices + s) * k1 + c) * N;
#pragma unroll
        for (int m = 0; m < E; m += 2) {
            const double2 p = *reinterpret_cast<const double2 *>(src + W::key_word(t, m));
            x[m] += p.x;
            x[m + 1] += p.y;
        }
    }
    W::inverse(x, xc, t, Twiddles(a.tw_inv + W::LANE_TABLE_OFFSET, a.tw_inv));
    const bool body = c + 1 == k1;
    const uint64_t *bodies = reinterpret_cast<const uint64_t *>(a.fields + (size_t)a.n * a.cols) + (size_t)g * N;   // zero past the fill
    __syncthreads();   // the transform is done with the exchange buffer: it takes the residues
    uint64_t *stage = reinterpret_cast<uint64_t *>(lds);
#pragma unroll
    for (int m = 0; m < E; m++) {
        const uint32_t j = W::template index_of<0>(t, m);
        uint64_t r = fq_neg(fp_to_u64(fp_canon(x[m])));
        if (body) r = fq_add(r, bodies[j]);
        stage[j] = r;
    }
    __syncthreads();
    uint64_t *dst = a.words + ((size_t)g * k1 + c) * N;
    for (uint32_t j = 2 * t; j < (uint32_t)N; j += 2 * LANES) *reinterpret_cast<u64x2 *>(dst + j) = *reinterpret_cast<const u64x2 *>(stage + j);
}

int dev_fold_front(const fbs_ctx *ctx, const uint64_t *d_cts, size_t count, uint32_t cols, uint32_t tg, uint32_t *d_fields, hipStream_t stream) {
    static_assert(256 % FF_COLS == 0 && 256 % FF_ROWS == 0, "D and the columns of a pass are multiples of N >= 256");
    hipLaunchKernelGGL(k_fold_front, dim3(ctx->D / FF_COLS, cols / FF_ROWS), dim3(256), 0, stream, d_cts, ctx->D, count, cols, tg, d_fields);
    FBS_HIP(ctx, hipGetLastError());
    return FBS_OK;
}

int dev_fold(fbs_ctx *ctx, const uint64_t *d_cts, size_t count, uint64_t *d_glwe, hipStream_t stream, const uint32_t *d_map, size_t n_src) {
    if (count == 0) return FBS_OK;
    const uint32_t N = ctx->N, D = ctx->D, k1 = ctx->p.k + 1;
    const size_t samples = (count + N - 1) / N;
    PackArgs a{};
    a.fields = ctx->d_pack_fields;
    a.key = ctx->gadget_dev[GK_FOLD].d_key;
    a.acc = ctx->d_pack_acc;
    a.tw_fwd = reinterpret_cast<const double *>(ctx->d_tw_fwd);
    a.tw_inv = reinterpret_cast<const double *>(ctx->d_tw_inv);
    a.words = d_glwe;
    a.count = count;
    a.sample_words = (size_t)k1 * N;
    a.n = D;
    a.t = ctx->gadget[GK_FOLD].t;
    a.gamma = ctx->gadget[GK_FOLD].gamma;
    a.cols = (uint32_t)(samples * N);
    a.slices = pack_slices_for(ctx, samples, D);
    if (((size_t)D + 2) * a.cols > ctx->pack_fields_capacity || samples * a.slices * k1 * N > ctx->pack_acc_capacity)
        return set_error(ctx, FBS_E_INVALID, "fold scratch too small for the launch");
    if (d_map) {
        hipLaunchKernelGGL(k_fold_front_mapped, dim3(D / FF_COLS, a.cols / FF_ROWS), dim3(256), 0, stream, d_cts, n_src, d_map, D, count,
                           a.cols, a.t * a.gamma, ctx->d_pack_fields);
        FBS_HIP(ctx, hipGetLastError());
    } else if (int rc = dev_fold_front(ctx, d_cts, count, a.cols, a.t * a.gamma, ctx->d_pack_fields, stream)) {
        return rc;
    }
    if (int rc = dev_pack_accumulate(ctx, a, samples, stream)) return rc;
    bool launched = false;
#define X(L, K1)                                                                                                                \
    if (ctx->p.log_n_poly == L && k1 == K1) {                                                                                   \
        hipLaunchKernelGGL((k_fold_finish<L, lanes_log2_for(L)>), dim3((unsigned)(samples * k1)), dim3(1 << lanes_log2_for(L)), 0, \
                           stream, a, k1);                                                                                      \
        launched = true;                                                                                                        \
    }
    X(8, 2) X(9, 2) X(10, 2) X(11, 2) X(12, 2) FBS_GLWE_SHAPES(X)
#undef X
    if (!launched) return set_error(ctx, FBS_E_INVALID, "no fold kernel for this (k, N)");
    FBS_HIP(ctx, hipGetLastError());
    return FBS_OK;
}

}  // namespace fbs

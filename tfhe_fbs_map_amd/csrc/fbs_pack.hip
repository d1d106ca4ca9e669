// Packed outputs (include/fbs_exec.h, "packed outputs"), gfx950: up to N small-key ciphertexts at 31 bits a field into the N
// coefficients of one GLWE sample under the big key -- a packing key switch on the transforms of fbs_ntt*.hpp and the FP64 field
// of fbs_field.hpp (no new arithmetic: every product is fp_mulmod, every sum an exact integer-valued double).
//
//   k_key_transform        (fbs_blind_rotate.hpp) the packing key [n][t_p][k+1][N], coefficient domain -> transform domain: once
//                          per key, the kernel that transforms the bootstrapping key.
//   k_pack_transpose       the switched fields of a pass, [ciphertext][n + 1] as the key switch leaves them, -> [n + 1][samples N]:
//                          a digit polynomial D_(i,v) is a COLUMN of the first matrix and a contiguous row segment of the second.
//                          64 x 64 tiles through LDS, coalesced 4-byte loads and stores both ways.  The mask fields are rounded to
//                          t_p gamma_p bits on the way (pack_round_mask); the body field is kept as it is; ciphertexts past the
//                          last one of a partly filled sample read as zero.
//   k_pack_accumulate      one workgroup = one packed sample, or one slice of its i range (launches of fewer samples than the chip
//                          has room for: pack_slices_for), on the lanes of ONE polynomial; the k + 1 accumulators live in
//                          registers in the transform domain.  Per (i, v): balanced digit of every coefficient (pack_digit),
//                          forward transform, k + 1 products with the key row.  The key row is requested (coalesced 16-byte loads,
//                          key_word order) before the transform that hides its latency; every workgroup of a slice walks i in the
//                          same order, so a row comes from HBM once per L2.  Partial accumulators leave centred, in register order.
//   k_pack_finish          one workgroup per (sample, component): the slices' partial accumulators summed mod q, inverse transform,
//                          ACC_c = -sum (c < k), ACC_k = lifted bodies - sum, transport rounding to w bits (compact_round), and the
//                          component's fields bit-packed from LDS (compact_word).  A component's fields start on a word boundary
//                          (N w is a multiple of 64), so the workgroups of a sample write disjoint words.
//
// Every value is an exact residue: the words do not depend on the number of slices or on the order of the sums.
// tests/test_gpu_pack_shapes.py holds that word for word against the definition restated in tests/helpers.py, on fields fed in
// through fbs_debug_pack_fields_dev (dev_pack below, without the key switch in front of it): every (k, N) of FBS_PACK_SHAPES at
// (t_p, gamma_p) = (3, 10) and the shipped (1, 27), fills 1, N - 1, N, N + 1, every slicing; (1, 31), (31, 1) and (2, 15) -- both
// branches of pack_round_mask, the widest digit, the most levels -- on one shape per transform class; n + 1 = 64, 65 and 735 columns
// through k_pack_transpose, stale rows behind `count`; two passes of fbs_pack_dev.  The fields are planted (planted_pack_fields): a
// mask field that rounds up and wraps, the rounding tie, -B/2 and B/2 - 1 on every level, the carry dropped at the top, the body
// fields either side of pack_lift_body's sign change.  tests/test_packed_reference.py holds the restatement to the host decode.
// Not reachable from the coefficient side: the lazy accumulator at its worst, 16 same-signed products near 0.8 q in the transform
// domain; that rests on the arithmetic stated at PACK_CENTRE_EVERY (16 x 0.8 q + q / 2 < 2^52).
// None of these is a key-switch or blind-rotation launch: they are not in fbs_kernel_catalog and the profile does not count them.
// k_pack_accumulate is generic in its row count and field source (PackArgs.n, fields, key: fbs_pack.hpp): folded state
// (fbs_fold.hip) launches it through dev_pack_accumulate with n := D, the fold's fields and the fold key, as it stands.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fbs_blind_rotate.hpp"
#include "fbs_pack.hpp"

namespace fbs {

constexpr uint32_t PACK_MAX_SLICES = 32;   // partial sums of centred residues: 32 x q/2 stays far below 2^52
constexpr uint32_t PACK_CENTRE_EVERY = 16; // lazy accumulators: 16 products below 0.8 q on top of q/2

// ms [count][n1] -> out [n1][cols], cols = samples * N a multiple of 64; grid (ceil(n1 / 64), cols / 64), 256 threads
__global__ __launch_bounds__(256) void k_pack_transpose(const uint32_t *__restrict__ ms, uint32_t n1, size_t count, uint32_t cols,
                                                        uint32_t tg, uint32_t *__restrict__ out) {
    __shared__ uint32_t tile[64][65];
    const uint32_t tx = threadIdx.x & 63u, ty = threadIdx.x >> 6;
    const uint32_t i0 = blockIdx.x * 64u, j0 = blockIdx.y * 64u;
    for (uint32_t r = ty; r < 64; r += 4) {
        const size_t j = (size_t)j0 + r;
        const uint32_t i = i0 + tx;
        tile[r][tx] = (j < count && i < n1) ? ms[j * n1 + i] : 0u;
    }
    __syncthreads();
    for (uint32_t r = ty; r < 64; r += 4) {
        const uint32_t i = i0 + r;
        if (i >= n1) break;
        const uint32_t x = tile[tx][r];
        out[(size_t)i * cols + j0 + tx] = i + 1 < n1 ? pack_round_mask(x, tg) : x;
    }
}

template <int LOGN, int LL, int K1>
__global__ __launch_bounds__(1 << LL) void k_pack_accumulate(PackArgs a) {
    using W = typename NttFor<LOGN, LL>::type;
    constexpr int N = W::N, E = W::E;
    __shared__ double lds[2 * N];
    const uint32_t t = threadIdx.x;
    const uint32_t g = blockIdx.x / a.slices, s = blockIdx.x % a.slices;
    const uint32_t i0 = (uint32_t)((uint64_t)s * a.n / a.slices), i1 = (uint32_t)((uint64_t)(s + 1) * a.n / a.slices);
    const uint32_t tg = a.t * a.gamma, offs = pack_digit_offsets(a.t, a.gamma), tg_mask = (uint32_t)((1ull << tg) - 1);
    typename W::Xchg xc{lds, 0};
    const Twiddles twf(a.tw_fwd + W::LANE_TABLE_OFFSET, a.tw_fwd);
    double acc[K1][E];
#pragma unroll
    for (int c = 0; c < K1; c++)
#pragma unroll
        for (int m = 0; m < E; m++) acc[c][m] = 0.0;
    uint32_t lazy = 0;
    for (uint32_t i = i0; i < i1; i++) {
        const uint32_t *col = a.fields + (size_t)i * a.cols + (size_t)g * N;
        uint32_t z[E];
#pragma unroll
        for (int m = 0; m < E; m++) z[m] = (col[W::template index_of<0>(t, m)] + offs) & tg_mask;
        for (uint32_t v = 0; v < a.t; v++) {
            // the key row first: its words arrive while the digits are transformed
            const double *row = a.key + ((size_t)i * a.t + v) * (size_t)K1 * N;
            double2 kw[K1][E / 2];
#pragma unroll
            for (int c = 0; c < K1; c++)
#pragma unroll
                for (int m = 0; m < E; m += 2) kw[c][m / 2] = *reinterpret_cast<const double2 *>(row + (size_t)c * N + W::key_word(t, m));
            double x[E];
#pragma unroll
            for (int m = 0; m < E; m++) x[m] = (double)pack_digit(z[m], v, a.t, a.gamma);
            W::forward(x, xc, t, twf);
#pragma unroll
            for (int c = 0; c < K1; c++)
#pragma unroll
                for (int m = 0; m < E; m += 2) {
                    acc[c][m] += fp_mulmod(x[m], kw[c][m / 2].x);
                    acc[c][m + 1] += fp_mulmod(x[m + 1], kw[c][m / 2].y);
                }
            if (++lazy == PACK_CENTRE_EVERY) {
                lazy = 0;
#pragma unroll
                for (int c = 0; c < K1; c++)
#pragma unroll
                    for (int m = 0; m < E; m++) acc[c][m] = fp_center(acc[c][m]);
            }
        }
    }
    double *dst = a.acc + (size_t)blockIdx.x * K1 * N;
#pragma unroll
    for (int c = 0; c < K1; c++)
#pragma unroll
        for (int m = 0; m < E; m += 2) {
            double2 o;
            o.x = fp_center(acc[c][m]);
            o.y = fp_center(acc[c][m + 1]);
            *reinterpret_cast<double2 *>(dst + (size_t)c * N + W::key_word(t, m)) = o;
        }
}

// grid: samples * (k + 1) workgroups, component fastest
template <int LOGN, int LL>
__global__ __launch_bounds__(1 << LL) void k_pack_finish(PackArgs a, uint32_t k1) {
    using W = typename NttFor<LOGN, LL>::type;
    constexpr int N = W::N, E = W::E, LANES = W::LANES;
    __shared__ double lds[2 * N];
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
    const uint32_t fill = (uint32_t)std::min<size_t>(N, a.count - (size_t)g * N);
    const uint32_t n_fields = body ? fill : (uint32_t)N;
    __syncthreads();   // the transform is done with the exchange buffer: it takes the rounded fields
    uint32_t *fields = reinterpret_cast<uint32_t *>(lds);
#pragma unroll
    for (int m = 0; m < E; m++) {
        const uint32_t j = W::template index_of<0>(t, m);
        uint64_t r = fq_neg(fp_to_u64(fp_canon(x[m])));
        if (body) r = fq_add(r, pack_lift_body(a.fields[(size_t)a.n * a.cols + (size_t)g * N + j]));
        fields[j] = compact_round(r, a.bits);
    }
    __syncthreads();
    uint64_t *dst = a.words + (size_t)g * a.sample_words + (size_t)c * N * a.bits / 64;
    const uint32_t Wc = (uint32_t)(((uint64_t)n_fields * a.bits + 63) / 64);
    for (uint32_t j = t; j < Wc; j += LANES) dst[j] = compact_word(j, n_fields, a.bits, [&](uint32_t f) { return fields[f]; });
}

// ---------------------------------------------------------------------------------------------
// the shapes a context can have (check_kernel_built): k = 1 at N = 256 .. 4096, and the GLWE shapes of fbs_select.hpp
#define FBS_PACK_SHAPES(X) X(8, 2) X(9, 2) X(10, 2) X(11, 2) X(12, 2) FBS_GLWE_SHAPES(X)

uint32_t pack_slices_for(const fbs_ctx *ctx, size_t samples, uint32_t rows) {
    const uint32_t cap = std::min<uint32_t>(PACK_MAX_SLICES, rows);
    if (ctx->tune.pack_slices > 0) return (uint32_t)std::min<int64_t>(ctx->tune.pack_slices, cap);
    // one wave per SIMD where a polynomial is one wave; a workgroup per CU where it is four
    const int ll = lanes_log2_for((int)ctx->p.log_n_poly);
    const size_t room = (size_t)std::max(1, ctx->cu_count) * (ll <= 6 ? 4 : ll == 7 ? 2 : 1);
    return (uint32_t)std::min<size_t>(cap, std::max<size_t>(1, room / std::max<size_t>(1, samples)));
}

// a key of rows x `t` GLWE rows (the packing key: n rows of the small key; the fold key: D words of the big key), whole
// and in the coefficient domain, -> the kind's d_key in the transform domain
int dev_upload_gadget_key(fbs_ctx *ctx, GadgetKind kind, const std::vector<uint64_t> &full, uint32_t t) {
    const uint32_t N = ctx->N, k1 = ctx->p.k + 1;
    const size_t polys = (size_t)gadget_rows(*ctx, kind) * t * k1, words = polys * N;
    double *&d_key = ctx->gadget_dev[kind].d_key;
    size_t &key_capacity = ctx->gadget_dev[kind].capacity;
    if (full.size() != words) return set_error(ctx, FBS_E_INVALID, "packing key of the wrong size");
    if (!ctx->d_tw_fwd) return set_error(ctx, FBS_E_STATE, "fbs_keygen has not run");
    if (ctx->scratch_used) FBS_HIP(ctx, hipStreamSynchronize(ctx->scratch_stream));   // kernels may still read the old key
    FBS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (words > key_capacity) {
        if (d_key) (void)hipFree(d_key);
        d_key = nullptr;
        key_capacity = 0;
        FBS_HIP(ctx, hipMalloc(&d_key, words * 8));
        key_capacity = words;
    }
    uint64_t *d_src = nullptr;
    FBS_HIP(ctx, hipMalloc(&d_src, words * 8));
    hipError_t e = hipMemcpyAsync(d_src, full.data(), words * 8, hipMemcpyHostToDevice, ctx->stream);
    const double n_inv = fq_centered(fq_inv(N));
    const unsigned grid = (unsigned)std::min<size_t>(polys, 4096);
    bool launched = false;
    if (e == hipSuccess) {
        switch (ctx->p.log_n_poly) {
#define X(L)                                                                                                                    \
    case L:                                                                                                                     \
        hipLaunchKernelGGL((k_key_transform<L, lanes_log2_for(L), KeyWords>), dim3(grid), dim3(1 << lanes_log2_for(L)), 0,     \
                           ctx->stream, KeyWords{d_src}, d_key, reinterpret_cast<const double *>(ctx->d_tw_fwd), n_inv, polys);               \
        launched = true;                                                                                                        \
        break;
            X(8) X(9) X(10) X(11) X(12)
#undef X
        }
        if (launched) e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    (void)hipFree(d_src);
    if (e != hipSuccess) return set_error(ctx, FBS_E_DEVICE, std::string("packing-key transform: ") + hipGetErrorString(e));
    if (!launched) return set_error(ctx, FBS_E_INVALID, "no packing kernel for this polynomial size");
    return FBS_OK;
}

// k_pack_accumulate on the fields, key and row count of `a` (a.n = n: packing; a.n = D: folding): samples * a.slices workgroups
int dev_pack_accumulate(const fbs_ctx *ctx, const PackArgs &a, size_t samples, hipStream_t stream) {
    const uint32_t k1 = ctx->p.k + 1;
    bool launched = false;
#define X(L, K1)                                                                                                                \
    if (ctx->p.log_n_poly == L && k1 == K1) {                                                                                   \
        hipLaunchKernelGGL((k_pack_accumulate<L, lanes_log2_for(L), K1>), dim3((unsigned)(samples * a.slices)),                 \
                           dim3(1 << lanes_log2_for(L)), 0, stream, a);                                                         \
        launched = true;                                                                                                        \
    }
    FBS_PACK_SHAPES(X)
#undef X
    if (!launched) return set_error(ctx, FBS_E_INVALID, "no packing kernel for this (k, N)");
    FBS_HIP(ctx, hipGetLastError());
    return FBS_OK;
}

int dev_pack(fbs_ctx *ctx, const uint32_t *d_ms, size_t count, uint32_t bits, uint64_t *d_words, hipStream_t stream) {
    if (count == 0) return FBS_OK;
    const uint32_t N = ctx->N, n = ctx->p.n, k1 = ctx->p.k + 1;
    const size_t samples = (count + N - 1) / N;
    PackArgs a{};
    a.fields = ctx->d_pack_fields;
    a.key = ctx->gadget_dev[GK_PACK].d_key;
    a.acc = ctx->d_pack_acc;
    a.tw_fwd = reinterpret_cast<const double *>(ctx->d_tw_fwd);
    a.tw_inv = reinterpret_cast<const double *>(ctx->d_tw_inv);
    a.words = d_words;
    a.count = count;
    a.sample_words = packed_sample_words(ctx->p.k, N, N, bits);
    a.n = n;
    a.t = ctx->gadget[GK_PACK].t;
    a.gamma = ctx->gadget[GK_PACK].gamma;
    a.cols = (uint32_t)(samples * N);
    a.slices = pack_slices_for(ctx, samples, n);
    a.bits = bits;
    if ((size_t)(n + 1) * a.cols > ctx->pack_fields_capacity || samples * a.slices * k1 * N > ctx->pack_acc_capacity)
        return set_error(ctx, FBS_E_INVALID, "packing scratch too small for the launch");
    hipLaunchKernelGGL(k_pack_transpose, dim3((n + 1 + 63) / 64, a.cols / 64), dim3(256), 0, stream, d_ms, n + 1, count, a.cols,
                       a.t * a.gamma, ctx->d_pack_fields);
    FBS_HIP(ctx, hipGetLastError());
    if (int rc = dev_pack_accumulate(ctx, a, samples, stream)) return rc;
    bool launched = false;
#define X(L, K1)                                                                                                                \
    if (ctx->p.log_n_poly == L && k1 == K1) {                                                                                   \
        hipLaunchKernelGGL((k_pack_finish<L, lanes_log2_for(L)>), dim3((unsigned)(samples * k1)), dim3(1 << lanes_log2_for(L)), 0, \
                           stream, a, k1);                                                                                      \
        launched = true;                                                                                                        \
    }
    FBS_PACK_SHAPES(X)
#undef X
    if (!launched) return set_error(ctx, FBS_E_INVALID, "no packing kernel for this (k, N)");
    FBS_HIP(ctx, hipGetLastError());
    return FBS_OK;
}

}  // namespace fbs

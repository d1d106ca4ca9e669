// The evaluation keys made and expanded on the device (knob "keys_on_device", include/fbs_exec.h), gfx950: word for word what
// host_keygen, host_keygen_seeded, host_expand_seeded_keys and host_gadget_keygen (fbs_host.cpp) write -- the same ChaCha20
// streams (fbs_chacha.hpp), the same folds, the same sampler (fbs_sampler.hpp), and the negacyclic product by the secret as an
// exact product of transforms (k_polymul's arithmetic: every value a residue, so the words do not depend on how it is computed).
//
//   k_key_transform<.., KeyBits>   (fbs_blind_rotate.hpp) the k polynomials of the GLWE secret, from its packed bits, in the form
//                        the bootstrapping key's transform has: once per call, into a buffer the caller zeroes and frees before it returns
//   k_glwe_key_rows      one GLWE key row per workgroup on the lanes of one polynomial (NttFor<LOGN, lanes_log2_for(LOGN)>): the
//                        mask columns from their stream (a lane makes whole 64-byte blocks), the body = sum_c A_c S_c + e + message.
//                        The transform's exchange buffer stages the mask words on their way into the lanes' registers and, after
//                        the inverse transform, the noise samples (four samples are exactly three blocks)
//   k_lwe_key_rows       one wave per key-switching row, on the frame of fbs_rows.hpp
//
// Rows leave in the standard coefficient layout of fbs_key_sizes.  None of these is a key-switch or blind-rotation launch: they
// are not in fbs_kernel_catalog and the profile does not count them.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fbs_blind_rotate.hpp"
#include "fbs_pack.hpp"
#include "fbs_rows.hpp"

namespace fbs {

// what a row of k_glwe_key_rows carries
enum KeyRowsMode : uint32_t {
    ROWS_FULL = 0,     // host_keygen: all k + 1 columns; bit g_lv on coefficient 0 of column comp
    ROWS_SEEDED = 1,   // host_keygen_seeded: all k + 1 columns; the message in the body whatever the component
    ROWS_PACK = 2,     // host_gadget_keygen: the body alone; sk_lwe[i] h_v on coefficient 0
    ROWS_EXPAND = 3    // host_expand_seeded_keys: the mask columns, then the given body; no secret
};

constexpr uint32_t KEY_ROWS_MAX_BLOCKS = 8192;   // grid cap; the workgroups (waves) stride over the rest
constexpr uint32_t LWE_ROWS_WAVES = 4;           // key-switching rows in flight per workgroup

struct GlweRowsArgs {
    uint64_t *dst;             // rows [n_rows][k + 1][N]; ROWS_PACK: bodies [n_rows][N]
    const uint64_t *bodies;    // ROWS_EXPAND: [n_rows][N]
    const double *s_hat;       // [k][N] the secret's transforms (launch_secret_transform)
    const double *tw_fwd, *tw_inv;
    const uint32_t *sk_glwe_bits, *sk_lwe_bits;
    RandKey mask_key, noise_key;
    Domain mask_dom, noise_dom;
    size_t n_rows;
    uint32_t mode, k, l, rows_per_sample, group, sampler;
    uint64_t sigma;
    uint64_t gadget[32];       // g_lv (l <= 16); ROWS_PACK: pack_gadget(gamma_p, v) (t_p <= 31, passed as l = rows_per_sample = t_p)
};

struct LweRowsArgs {
    uint64_t *dst;             // rows [n_rows][n + 1]
    const uint64_t *bodies;    // non-null: the expand mode, [n_rows]
    const uint32_t *sk_glwe_bits, *sk_lwe_bits;
    RandKey mask_key, noise_key;
    Domain mask_dom, noise_dom;
    size_t n_rows;
    uint32_t n, t, sampler;
    uint64_t sigma;
    uint64_t h[64];            // h_v
};

__device__ __forceinline__ bool packed_bit(const uint32_t *bits, size_t i) { return (bits[i >> 5] >> (i & 31u)) & 1u; }

// the bit GGSW sample g encrypts (ggsw_bit, fbs_host.cpp)
__device__ __forceinline__ bool ggsw_bit_dev(const uint32_t *sk_lwe_bits, uint32_t group, size_t g) {
    if (group != 2) return packed_bit(sk_lwe_bits, g);
    const bool s0 = packed_bit(sk_lwe_bits, 2 * (g / 3)), s1 = packed_bit(sk_lwe_bits, 2 * (g / 3) + 1);
    return g % 3 == 0 ? (s0 && !s1) : g % 3 == 1 ? (!s0 && s1) : (s0 && s1);
}

template <int LOGN, int LL>
__global__ __launch_bounds__(1 << LL) void k_glwe_key_rows(GlweRowsArgs a) {
    using W = typename NttFor<LOGN, LL>::type;
    constexpr int N = W::N, E = W::E, LANES = W::LANES;
    __shared__ __attribute__((aligned(16))) double lds[2 * N];
    uint64_t *stage = reinterpret_cast<uint64_t *>(lds);   // N words of the exchange buffer, between transforms
    const uint32_t t = threadIdx.x, k = a.k;
    typename W::Xchg xc{lds, 0};
    const Twiddles twf(a.tw_fwd + W::LANE_TABLE_OFFSET, a.tw_fwd), twi(a.tw_inv + W::LANE_TABLE_OFFSET, a.tw_inv);
    const bool full_row = a.mode != ROWS_PACK;
    for (size_t r = blockIdx.x; r < a.n_rows; r += gridDim.x) {   // uniform per workgroup
        const size_t g = r / a.rows_per_sample;
        const uint32_t rr = (uint32_t)(r % a.rows_per_sample), comp = rr / a.l, lv = rr % a.l;
        uint64_t *row = a.dst + r * (full_row ? (size_t)(k + 1) * N : (size_t)N);
        uint64_t *body = full_row ? row + (size_t)k * N : row;
        const uint64_t mask_stream = stream_id(a.mask_dom, r), noise_stream = stream_id(a.noise_dom, r);
        bool bit = false;
        if (a.mode == ROWS_PACK) bit = packed_bit(a.sk_lwe_bits, g);
        else if (a.mode != ROWS_EXPAND) bit = ggsw_bit_dev(a.sk_lwe_bits, a.group, g);
        const uint64_t msg = a.gadget[lv];

        double acc[E];
#pragma unroll
        for (int m = 0; m < E; m++) acc[m] = 0.0;
        for (uint32_t c = 0; c < k; c++) {
            __syncthreads();   // whoever read the exchange buffer last is done
            // column c: words c N .. c N + N - 1 of the mask stream, N a multiple of 8: whole blocks
            for (uint32_t b = t; b < (uint32_t)N / 8; b += LANES) {
                uint64_t w[8];
                chacha_block(a.mask_key.w, mask_stream, (uint64_t)c * (N / 8) + b, w);
                for (int i = 0; i < 8; i++) w[i] = fq_fold(w[i]);
                for (int i = 0; i < 8; i += 2) *reinterpret_cast<u64x2 *>(stage + 8 * b + i) = u64x2{w[i], w[i + 1]};
                if (full_row) {
                    // fbs_keygen's message sits on the mask column; the product below takes the column without it
                    if (a.mode == ROWS_FULL && bit && c == comp && b == 0) w[0] = fq_add(w[0], msg);
                    uint64_t *p = row + (size_t)c * N + 8 * (size_t)b;
                    for (int i = 0; i < 8; i += 2) *reinterpret_cast<u64x2 *>(p + i) = u64x2{w[i], w[i + 1]};
                }
            }
            if (a.mode == ROWS_EXPAND) continue;
            __syncthreads();
            double x[E];
#pragma unroll
            for (int m = 0; m < E; m++) x[m] = fp_from_u64(stage[W::template index_of<0>(t, m)]);
            __syncthreads();   // the staged words are in registers: the transform may have the buffer
            W::forward(x, xc, t, twf);
            // products below 0.8 q each, k <= 4 of them: far inside what the inverse transform accepts
            const double *s = a.s_hat + (size_t)c * N;
#pragma unroll
            for (int m = 0; m < E; m += 2) {
                const double2 sw = *reinterpret_cast<const double2 *>(s + W::key_word(t, m));
                acc[m] += fp_mulmod(x[m], sw.x);
                acc[m + 1] += fp_mulmod(x[m + 1], sw.y);
            }
        }
        if (a.mode == ROWS_EXPAND) {
#pragma unroll
            for (int m = 0; m < E; m++) {
                const uint32_t j = W::template index_of<0>(t, m);
                body[j] = a.bodies[r * N + j];
            }
            continue;
        }
        W::inverse(acc, xc, t, twi);   // (the 1 / N is in s_hat)
        uint64_t v[E];
#pragma unroll
        for (int m = 0; m < E; m++) v[m] = fp_to_u64(fp_canon(acc[m]));
        if (a.sigma) {
            __syncthreads();   // the transform is done with the exchange buffer: it takes the noise
            // samples 4 q .. 4 q + 3 own words 24 q .. 24 q + 23 of the noise stream: blocks 3 q, 3 q + 1, 3 q + 2
            for (uint32_t q = t; q < (uint32_t)N / 4; q += LANES) {
                uint64_t w[24];
                for (int i = 0; i < 3; i++) chacha_block(a.noise_key.w, noise_stream, 3ull * q + i, w + 8 * i);
                uint64_t e[4];
                for (int i = 0; i < 4; i++) e[i] = fq_from_i64(sample_window(a.sampler, w + 6 * i, a.sigma));
                *reinterpret_cast<u64x2 *>(stage + 4 * q) = u64x2{e[0], e[1]};
                *reinterpret_cast<u64x2 *>(stage + 4 * q + 2) = u64x2{e[2], e[3]};
            }
            __syncthreads();
#pragma unroll
            for (int m = 0; m < E; m++) v[m] = fq_add(v[m], stage[W::template index_of<0>(t, m)]);
        }
        if (bit) {
            if (a.mode == ROWS_SEEDED && comp < k) {   // -g_lv S_comp
#pragma unroll
                for (int m = 0; m < E; m++)
                    if (packed_bit(a.sk_glwe_bits, (size_t)comp * N + W::template index_of<0>(t, m))) v[m] = fq_sub(v[m], msg);
            } else if ((a.mode != ROWS_FULL || comp == k) && t == 0) {   // coefficient 0 is register 0 of lane 0
                v[0] = fq_add(v[0], msg);
            }
        }
#pragma unroll
        for (int m = 0; m < E; m++) body[W::template index_of<0>(t, m)] = v[m];
    }
}

__global__ __launch_bounds__(64 * LWE_ROWS_WAVES) void k_lwe_key_rows(LweRowsArgs a) {
    const uint32_t lane = threadIdx.x & 63u, n = a.n;
    for (size_t r = (size_t)blockIdx.x * LWE_ROWS_WAVES + threadIdx.x / 64; r < a.n_rows; r += (size_t)gridDim.x * LWE_ROWS_WAVES) {   // wave-uniform
        uint64_t *row = a.dst + r * (size_t)(n + 1);
        // n is any number: the one caller of the frame whose rows end in a partial block
        uint64_t sum = lwe_mask_row<true>(a.mask_key, stream_id(a.mask_dom, r), n, row, a.bodies ? nullptr : a.sk_lwe_bits, lane);
        if (a.bodies) {
            if (lane == 63) row[n] = a.bodies[r];
            continue;
        }
        sum = wave_sum(sum);
        if (lane == 63) {   // (the lane with the least mask work when the blocks do not fill the last round)
            const size_t j = r / a.t;
            const uint32_t v = (uint32_t)(r % a.t);
            uint64_t body = fq_add(sum % FQ, lwe_noise(a.noise_key, stream_id(a.noise_dom, r), a.sampler, a.sigma));
            if (packed_bit(a.sk_glwe_bits, j)) body = fq_add(body, a.h[v]);
            row[n] = body;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------
namespace {
struct DevBuf {   // a temporary device buffer of one call
    void *p = nullptr;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
    template <class T>
    T *as() const { return static_cast<T *>(p); }
};
}  // namespace

#define FBS_FOR_EACH_SHAPE(X) X(8) X(9) X(10) X(11) X(12)

// the secret's transforms -> s_hat (allocated here; the caller zeroes it before it is freed)
static int launch_secret_transform(fbs_ctx *ctx, DevBuf &s_hat) {
    const uint32_t N = ctx->N, k = ctx->p.k;
    FBS_HIP(ctx, hipMalloc(&s_hat.p, (size_t)k * N * 8));
    const double n_inv = fq_centered(fq_inv(N));
    const double *twf = reinterpret_cast<const double *>(ctx->d_tw_fwd);
    switch (ctx->p.log_n_poly) {
#define X(L)                                                                                                                    \
    case L:                                                                                                                     \
        hipLaunchKernelGGL((k_key_transform<L, lanes_log2_for(L), KeyBits>), dim3(k), dim3(1 << lanes_log2_for(L)), 0, ctx->stream, \
                           KeyBits{ctx->d_sk_bits}, s_hat.as<double>(), twf, n_inv, (size_t)k);   /* one workgroup per polynomial */ \
        break;
        FBS_FOR_EACH_SHAPE(X)
#undef X
        default: return set_error(ctx, FBS_E_INVALID, "unsupported N");
    }
    FBS_HIP(ctx, hipGetLastError());
    return FBS_OK;
}

static int launch_glwe_rows(fbs_ctx *ctx, const GlweRowsArgs &a) {
    const unsigned grid = (unsigned)std::min<size_t>(a.n_rows, KEY_ROWS_MAX_BLOCKS);
    switch (ctx->p.log_n_poly) {
#define X(L)                                                                                                                    \
    case L:                                                                                                                     \
        hipLaunchKernelGGL((k_glwe_key_rows<L, lanes_log2_for(L)>), dim3(grid), dim3(1 << lanes_log2_for(L)), 0, ctx->stream, a); \
        break;
        FBS_FOR_EACH_SHAPE(X)
#undef X
        default: return set_error(ctx, FBS_E_INVALID, "unsupported N");
    }
    FBS_HIP(ctx, hipGetLastError());
    return FBS_OK;
}

// the secret's transforms go back to zero before their buffer is freed
static int wipe(fbs_ctx *ctx, DevBuf &s_hat, size_t bytes) {
    if (!s_hat.p) return FBS_OK;
    FBS_HIP(ctx, hipMemsetAsync(s_hat.p, 0, bytes, ctx->stream));
    FBS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return FBS_OK;
}

int dev_make_keys(fbs_ctx *ctx, bool seeded, const RandKey &mask_key, const uint64_t *bsk_bodies, const uint64_t *ksk_bodies) {
    const fbs_params &p = ctx->p;
    const uint32_t N = ctx->N, n = p.n, k = p.k;
    const bool expand = bsk_bodies != nullptr;
    const size_t bsk_rows = ctx->n_ggsw * ctx->rows, row_words = (size_t)(k + 1) * N, ksk_rows = (size_t)ctx->D * p.t_ksk;
    DevBuf bsk, ksk, s_hat, d_bb, d_kb;
    FBS_HIP(ctx, hipMalloc(&bsk.p, bsk_rows * row_words * 8));
    FBS_HIP(ctx, hipMalloc(&ksk.p, ksk_rows * (size_t)(n + 1) * 8));
    if (expand) {
        FBS_HIP(ctx, hipMalloc(&d_bb.p, bsk_rows * N * 8));
        FBS_HIP(ctx, hipMalloc(&d_kb.p, ksk_rows * 8));
        FBS_HIP(ctx, hipMemcpyAsync(d_bb.p, bsk_bodies, bsk_rows * N * 8, hipMemcpyHostToDevice, ctx->stream));
        FBS_HIP(ctx, hipMemcpyAsync(d_kb.p, ksk_bodies, ksk_rows * 8, hipMemcpyHostToDevice, ctx->stream));
    } else if (int rc = launch_secret_transform(ctx, s_hat)) {
        return rc;
    }

    GlweRowsArgs ga{};
    ga.dst = bsk.as<uint64_t>();
    ga.bodies = d_bb.as<uint64_t>();
    ga.s_hat = s_hat.as<double>();
    ga.tw_fwd = reinterpret_cast<const double *>(ctx->d_tw_fwd);
    ga.tw_inv = reinterpret_cast<const double *>(ctx->d_tw_inv);
    ga.sk_glwe_bits = ctx->d_sk_bits;
    ga.sk_lwe_bits = ctx->d_sk_lwe_bits;
    ga.mask_key = seeded ? mask_key : ctx->rkey;
    ga.noise_key = ctx->rkey;
    ga.mask_dom = seeded ? DOM_SBSK_MASK : DOM_BSK_MASK;
    ga.noise_dom = seeded ? DOM_SBSK_NOISE : DOM_BSK_NOISE;
    ga.n_rows = bsk_rows;
    ga.mode = expand ? ROWS_EXPAND : seeded ? ROWS_SEEDED : ROWS_FULL;
    ga.k = k;
    ga.l = p.l_bsk;
    ga.rows_per_sample = ctx->rows;
    ga.group = ctx->group;
    ga.sampler = p.sampler;
    ga.sigma = p.sigma_glwe;
    for (uint32_t lv = 0; lv < p.l_bsk; lv++) ga.gadget[lv] = ctx->g[lv];

    LweRowsArgs la{};
    la.dst = ksk.as<uint64_t>();
    la.bodies = d_kb.as<uint64_t>();
    la.sk_glwe_bits = ctx->d_sk_bits;
    la.sk_lwe_bits = ctx->d_sk_lwe_bits;
    la.mask_key = ga.mask_key;
    la.noise_key = ctx->rkey;
    la.mask_dom = seeded ? DOM_SKSK_MASK : DOM_KSK_MASK;
    la.noise_dom = seeded ? DOM_SKSK_NOISE : DOM_KSK_NOISE;
    la.n_rows = ksk_rows;
    la.n = n;
    la.t = p.t_ksk;
    la.sampler = p.sampler;
    la.sigma = p.sigma_lwe;
    for (uint32_t v = 0; v < p.t_ksk; v++) la.h[v] = ctx->h[v];

    int rc = bsk_rows ? launch_glwe_rows(ctx, ga) : FBS_OK;
    if (rc == FBS_OK && ksk_rows) {
        const unsigned grid = (unsigned)std::min<size_t>((ksk_rows + LWE_ROWS_WAVES - 1) / LWE_ROWS_WAVES, KEY_ROWS_MAX_BLOCKS);
        hipLaunchKernelGGL(k_lwe_key_rows, dim3(grid), dim3(64 * LWE_ROWS_WAVES), 0, ctx->stream, la);
        if (hipGetLastError() != hipSuccess) rc = set_error(ctx, FBS_E_DEVICE, "key-switching-key rows: launch failed");
    }
    // the transforms straight from the device rows: the bootstrapping key is not uploaded again
    if (rc == FBS_OK) rc = dev_transform_bsk(ctx, bsk.as<uint64_t>());
    const int wiped = wipe(ctx, s_hat, (size_t)k * N * 8);
    if (rc != FBS_OK) return rc;
    if (wiped != FBS_OK) return wiped;
    // the host copies, which every export and every derived key-switching table reads
    ctx->bsk.resize(bsk_rows * row_words);
    ctx->ksk.resize(ksk_rows * (size_t)(n + 1));
    FBS_HIP(ctx, hipMemcpy(ctx->bsk.data(), bsk.p, ctx->bsk.size() * 8, hipMemcpyDeviceToHost));
    FBS_HIP(ctx, hipMemcpy(ctx->ksk.data(), ksk.p, ctx->ksk.size() * 8, hipMemcpyDeviceToHost));
    return FBS_OK;
}

// bodies [rows][t][N] of host_gadget_keygen (fbs_host.cpp): ROWS_PACK rows whose bit is bit i of the kind's secret on the device
int dev_gadget_bodies(fbs_ctx *ctx, GadgetKind kind, uint32_t t, uint32_t gamma, std::vector<uint64_t> &bodies) {
    const uint32_t N = ctx->N, k = ctx->p.k;
    const size_t n_rows = (size_t)gadget_rows(*ctx, kind) * t;
    if (!ctx->d_tw_fwd || !ctx->d_sk_bits) return set_error(ctx, FBS_E_STATE, "fbs_keygen has not run");
    bodies.assign(n_rows * N, 0);
    if (!n_rows) return FBS_OK;
    DevBuf d_bodies, s_hat;
    FBS_HIP(ctx, hipMalloc(&d_bodies.p, n_rows * N * 8));
    if (int rc = launch_secret_transform(ctx, s_hat)) return rc;
    GlweRowsArgs ga{};
    ga.dst = d_bodies.as<uint64_t>();
    ga.s_hat = s_hat.as<double>();
    ga.tw_fwd = reinterpret_cast<const double *>(ctx->d_tw_fwd);
    ga.tw_inv = reinterpret_cast<const double *>(ctx->d_tw_inv);
    ga.sk_glwe_bits = ctx->d_sk_bits;
    // (ROWS_PACK reads the bit of "sample" i here: the small key's, or for the fold key the big key's)
    ga.sk_lwe_bits = kind == GK_PACK ? ctx->d_sk_lwe_bits : ctx->d_sk_bits;
    ga.mask_key = ctx->mask_key;
    ga.noise_key = ctx->rkey;
    ga.mask_dom = GADGET_KINDS[kind].mask_dom;
    ga.noise_dom = GADGET_KINDS[kind].noise_dom;
    ga.n_rows = n_rows;
    ga.mode = ROWS_PACK;
    ga.k = k;
    ga.l = ga.rows_per_sample = t;   // row r = i t + v: "sample" i, level v
    ga.group = 1;
    ga.sampler = ctx->p.sampler;
    ga.sigma = ctx->p.sigma_glwe;
    for (uint32_t v = 0; v < t; v++) ga.gadget[v] = pack_gadget(gamma, v);
    int rc = launch_glwe_rows(ctx, ga);
    if (rc == FBS_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = set_error(ctx, FBS_E_DEVICE, "packing-key rows failed");
    const int wiped = wipe(ctx, s_hat, (size_t)k * N * 8);
    if (rc != FBS_OK) return rc;
    if (wiped != FBS_OK) return wiped;
    FBS_HIP(ctx, hipMemcpy(bodies.data(), d_bodies.p, bodies.size() * 8, hipMemcpyDeviceToHost));
    return FBS_OK;
}

}  // namespace fbs

// Audited evaluation (include/fbs_exec.h, "audited evaluation"), gfx950: ciphertexts plus the messages they should hold -> exact
// error statistics, on the device, under the secret keys the context already keeps there (d_sk_bits, d_sk_lwe_bits).
//
//   k_audit_wire     big-key ciphertexts in their wire slots.  One wave per (row, sample), the structure of k_decrypt
//                    (fbs_io.hip): lanes striding the mask, the key-selected words in a 64-bit sum (D words below 2^46: below
//                    2^58), the wave's sum reduced once, phase = b - sum mod q.  With m = expected mod 2p in [0, 2p) and
//                    Delta = 2 delta_half the error is e = centred((phase - Delta m) mod q), an int64 in [-(q-1)/2, (q-1)/2].
//                    Loads are coalesced 8-byte loads: D + 1 is odd, so every other ciphertext starts on an odd word and 16-byte
//                    loads would need k_encrypt's two layouts; at 8 bytes a lane one wave load is 512 contiguous bytes and the
//                    kernel is bound by HBM either way.
//   k_audit_fields   the (n + 1) 32-bit fields the key switch at width log2(2N) leaves in the modulus-switched scratch -- what the
//                    blind rotation reads and k_compact_pack packs.  One wave per (source, sample), the structure of
//                    k_decrypt_compact (fbs_compact.hip): coalesced 4-byte loads, a 32-bit sum of the fields whose small-key bit is
//                    set (exact mod 2^32, hence mod 2N), ph = (body - sum) mod 2N in [0, 2N) -- the phase fbs_decrypt_compact
//                    decodes at w = log2(2N).  e = centred((2p ph - 2N m) mod 4pN) in [-2pN, 2pN): the torus error is e / (4pN)
//                    and the half box 1/(4p) is N of these units.  This takes 2p Delta for q: Delta = 2 round(q / 4p), so
//                    |2p Delta - q| <= 2p, a relative difference of the box of at most 2p/q < 4p/q (below 2^-32 at p <= 4096),
//                    far below one unit, 1/(4pN), of this scale.
//   k_audit_reduce   one workgroup per row over its s_count errors: count, the samples at half a box or beyond (`over`), max |e|,
//                    sum (int64) and sum of squares (128 bits in two words).  Integer arithmetic only, no floating point and no
//                    atomics: every partial sum is an exact integer mod 2^64 / 2^128 and addition there is associative and
//                    commutative, so the result does not depend on the order and is bit-reproducible.  Per lane the squares
//                    (|e| < 2^45: a square below 2^90, from a 64 x 64 -> 128 product) are added with carry; waves combine by
//                    __shfl_xor with the carry of the low word propagated at every step, workgroups through LDS (one slot per
//                    wave: no conflicts), added up by one lane.  s_count <= AUDIT_MAX_SAMPLES = 2^18 per call (the launcher
//                    refuses more): |sum| <= 2^18 (2^45 - 1) < 2^63 and sumsq < 2^108, so neither can overflow.
//
// None is a key-switch or blind-rotation launch: they are not in fbs_kernel_catalog and the profile does not count them.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fbs_rows.hpp"

namespace fbs {

constexpr uint32_t AUDIT_WAVES = 4;              // waves (ciphertexts in flight) per workgroup
constexpr uint32_t AUDIT_MAX_BLOCKS = 1u << 16;  // grid cap; the waves stride over the rest
constexpr uint32_t AUDIT_REDUCE_WAVES = 4;

struct AuditWireArgs {
    const uint64_t *wires;
    const uint32_t *row_slot;   // [rows] wire slot of each row
    const int64_t *expected;    // [rows][s_count]
    int64_t *err;               // [rows][s_count]
    size_t rows, T, s_begin, s_count;
    const uint32_t *sk;         // GLWE secret key, packed bits
    uint32_t D;
    uint64_t two_p, delta;
};

struct AuditFieldArgs {
    const uint32_t *ms;         // [rows * s_count][n + 1]
    const int64_t *expected;    // [rows][s_count]
    int64_t *err;               // [rows][s_count]
    size_t total;               // rows * s_count
    const uint32_t *sk;         // small LWE key, packed bits
    uint32_t n, log2_2n;
    uint64_t two_p;
};

// x mod two_p in [0, two_p) for any int64 (C++ % truncates towards zero)
__device__ __forceinline__ uint64_t audit_message(int64_t x, uint64_t two_p) {
    const int64_t r = x % (int64_t)two_p;
    return (uint64_t)(r < 0 ? r + (int64_t)two_p : r);
}

__global__ __launch_bounds__(64 * AUDIT_WAVES) void k_audit_wire(AuditWireArgs a) {
    const uint32_t lane = threadIdx.x & 63u, D = a.D;
    const size_t total = a.rows * a.s_count;
    for (size_t c = (size_t)blockIdx.x * AUDIT_WAVES + threadIdx.x / 64; c < total; c += (size_t)gridDim.x * AUDIT_WAVES) {   // wave-uniform
        const size_t r = c / a.s_count, s = c - r * a.s_count;
        const uint64_t *ct = a.wires + ((size_t)a.row_slot[r] * a.T + a.s_begin + s) * (D + 1);
        uint64_t sum = 0;
        for (uint32_t j = lane; j < D; j += 64) {
            const uint64_t w = ct[j];
            sum += ((a.sk[j >> 5] >> (j & 31u)) & 1u) ? w : 0;
        }
        sum = wave_sum(sum);
        if (lane == 0) {
            const uint64_t phase = fq_sub(ct[D], sum % FQ);
            const uint64_t want = (audit_message(a.expected[c], a.two_p) * a.delta) % FQ;   // < 2^13 2^46: no overflow
            const uint64_t x = fq_sub(phase, want);
            a.err[c] = x > (FQ - 1) / 2 ? (int64_t)x - (int64_t)FQ : (int64_t)x;
        }
    }
}

__global__ __launch_bounds__(64 * AUDIT_WAVES) void k_audit_fields(AuditFieldArgs a) {
    const uint32_t lane = threadIdx.x & 63u, mask = (1u << a.log2_2n) - 1u;
    for (size_t c = (size_t)blockIdx.x * AUDIT_WAVES + threadIdx.x / 64; c < a.total; c += (size_t)gridDim.x * AUDIT_WAVES) {   // wave-uniform
        const uint32_t *row = a.ms + c * (a.n + 1);
        uint32_t sum = 0;   // mod 2^32, hence mod 2N
        for (uint32_t i = lane; i < a.n; i += 64) {
            const uint32_t f = row[i];
            sum += ((a.sk[i >> 5] >> (i & 31u)) & 1u) ? f : 0;
        }
        sum = wave_sum(sum);
        if (lane == 0) {
            const uint64_t ph = (row[a.n] - sum) & mask;                       // [0, 2N)
            const uint64_t two_n = (uint64_t)mask + 1, box = a.two_p * two_n;  // 4pN <= 2^13 2^13
            const uint64_t x = (a.two_p * ph + box - two_n * audit_message(a.expected[c], a.two_p)) % box;
            a.err[c] = x >= box / 2 ? (int64_t)x - (int64_t)box : (int64_t)x;
        }
    }
}

// (lo, hi) += (olo, ohi) mod 2^128
__device__ __forceinline__ void add128(uint64_t &lo, uint64_t &hi, uint64_t olo, uint64_t ohi) {
    lo += olo;
    hi += ohi + (lo < olo ? 1u : 0u);
}

// over: mul |e| >= thr (wires: 4p |e| >= q; fields: |e| >= N)
__global__ __launch_bounds__(64 * AUDIT_REDUCE_WAVES) void k_audit_reduce(const int64_t *err, size_t s_count, uint64_t mul, uint64_t thr,
                                                                          fbs_audit_row *stats) {
    __shared__ uint64_t part[AUDIT_REDUCE_WAVES][5];
    const int64_t *row = err + (size_t)blockIdx.x * s_count;
    uint64_t over = 0, max_abs = 0, sum = 0, sq_lo = 0, sq_hi = 0;   // sum: two's complement, added mod 2^64
    for (size_t s = threadIdx.x; s < s_count; s += 64 * AUDIT_REDUCE_WAVES) {
        const int64_t e = row[s];
        const uint64_t m = e < 0 ? (uint64_t)(-e) : (uint64_t)e;
        over += (m * mul >= thr) ? 1u : 0u;   // |e| < 2^45, mul <= 2^14
        max_abs = m > max_abs ? m : max_abs;
        sum += (uint64_t)e;
        add128(sq_lo, sq_hi, m * m, __umul64hi(m, m));
    }
    for (int d = 32; d >= 1; d >>= 1) {
        over += __shfl_xor(over, d);
        const uint64_t om = __shfl_xor(max_abs, d);
        max_abs = om > max_abs ? om : max_abs;
        sum += __shfl_xor(sum, d);
        const uint64_t olo = __shfl_xor(sq_lo, d), ohi = __shfl_xor(sq_hi, d);
        add128(sq_lo, sq_hi, olo, ohi);
    }
    const uint32_t wave = threadIdx.x / 64;
    if ((threadIdx.x & 63u) == 0) {
        part[wave][0] = over;
        part[wave][1] = max_abs;
        part[wave][2] = sum;
        part[wave][3] = sq_lo;
        part[wave][4] = sq_hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t w = 1; w < AUDIT_REDUCE_WAVES; w++) {
            over += part[w][0];
            max_abs = part[w][1] > max_abs ? part[w][1] : max_abs;
            sum += part[w][2];
            add128(sq_lo, sq_hi, part[w][3], part[w][4]);
        }
        fbs_audit_row out;
        out.count = s_count;
        out.over = over;
        out.max_abs = max_abs;
        out.sum = (int64_t)sum;
        out.sumsq_lo = sq_lo;
        out.sumsq_hi = sq_hi;
        stats[blockIdx.x] = out;
    }
}

static dim3 audit_grid(size_t total) { return dim3((unsigned)std::min<size_t>((total + AUDIT_WAVES - 1) / AUDIT_WAVES, AUDIT_MAX_BLOCKS)); }

int dev_audit_wire(const fbs_ctx *ctx, const uint64_t *d_wires, const uint32_t *d_row_slot, size_t rows, size_t T, size_t s_begin,
                   size_t s_count, const int64_t *d_expected, int64_t *d_err, hipStream_t stream) {
    if (rows * s_count == 0) return FBS_OK;
    AuditWireArgs a{};
    a.wires = d_wires;
    a.row_slot = d_row_slot;
    a.expected = d_expected;
    a.err = d_err;
    a.rows = rows;
    a.T = T;
    a.s_begin = s_begin;
    a.s_count = s_count;
    a.sk = ctx->d_sk_bits;
    a.D = ctx->D;
    a.two_p = 2ull * ctx->p.p_msg;
    a.delta = 2 * ctx->delta_half;
    hipLaunchKernelGGL(k_audit_wire, audit_grid(rows * s_count), dim3(64 * AUDIT_WAVES), 0, stream, a);
    FBS_HIP(ctx, hipGetLastError());
    return FBS_OK;
}

int dev_audit_fields(const fbs_ctx *ctx, const uint32_t *d_ms, size_t rows, size_t s_count, const int64_t *d_expected, int64_t *d_err,
                     hipStream_t stream) {
    if (rows * s_count == 0) return FBS_OK;
    AuditFieldArgs a{};
    a.ms = d_ms;
    a.expected = d_expected;
    a.err = d_err;
    a.total = rows * s_count;
    a.sk = ctx->d_sk_lwe_bits;
    a.n = ctx->p.n;
    a.log2_2n = ctx->p.log_n_poly + 1;
    a.two_p = 2ull * ctx->p.p_msg;
    hipLaunchKernelGGL(k_audit_fields, audit_grid(a.total), dim3(64 * AUDIT_WAVES), 0, stream, a);
    FBS_HIP(ctx, hipGetLastError());
    return FBS_OK;
}

int dev_audit_reduce(const fbs_ctx *ctx, const int64_t *d_err, size_t rows, size_t s_count, bool fields, fbs_audit_row *d_stats,
                     hipStream_t stream) {
    if (rows == 0 || s_count == 0) return FBS_OK;
    if (s_count > AUDIT_MAX_SAMPLES) return set_error(ctx, FBS_E_INVALID, "more than 2^18 samples in one audit call (the 64-bit sum of errors could overflow)");
    if (rows > 0x7FFFFFFFull) return set_error(ctx, FBS_E_INVALID, "more than 2^31 rows in one launch");
    const uint64_t mul = fields ? 1 : 4ull * ctx->p.p_msg, thr = fields ? ctx->N : FQ;
    hipLaunchKernelGGL(k_audit_reduce, dim3((unsigned)rows), dim3(64 * AUDIT_REDUCE_WAVES), 0, stream, d_err, s_count, mul, thr, d_stats);
    FBS_HIP(ctx, hipGetLastError());
    return FBS_OK;
}

}  // namespace fbs

// Blind rotation + sample extraction (the hot kernel), the one-time key transform and a debug product, all on
// the NTT of fbs_ntt.hpp / fbs_ntt_split.hpp.  gfx950 only.  Exact modular arithmetic on integer-valued doubles (fbs_field.hpp): the
// FP64 FMA is the machine's widest exact multiplier; no MFMA, no tensor contraction -- every product is an
// element-wise residue product.
//
// One functional bootstrap = two waves (or 2 x LANES/64) of a workgroup; GLWE component c (k = 1: mask, body) is owned by LANES lanes, each
// holding E coefficients of the accumulator in VGPRs.  Per CMUX step: accumulator -> LDS, gather the rotated copy
// (X^a), subtract, round to l*beta bits; per digit level: balanced digit -> forward NTT -> multiply-accumulate with
// the two key polynomials of that row (lazy sums); hand the partner component its half through LDS; inverse NTT;
// accumulate and canonicalise.  The bootstrapping-key row of a step (96 KB at P1024) is read once per workgroup
// with 16-byte coalesced loads; all workgroups walk the key in step, so after the first touch it is served from
// L2/MALL, not HBM.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>
#include <utility>

#include "fbs_blind_rotate.hpp"

namespace fbs {

// ---------------------------------------------------------------------------------------------
template <int LOGN, int LL>
__global__ __launch_bounds__(1 << LL) void k_polymul(const uint64_t *a, const uint64_t *b, uint64_t *c, const double *tw_fwd,
                                                     const double *tw_inv, double n_inv) {
    using W = typename NttFor<LOGN, LL>::type;
    __shared__ double lds[2 * W::N];
    const uint32_t t = threadIdx.x;
    typename W::Xchg xc{lds, 0};
    double x[W::E], y[W::E];
#pragma unroll
    for (int m = 0; m < W::E; m++) {
        x[m] = fp_from_u64(a[W::template index_of<0>(t, m)]);
        y[m] = fp_from_u64(b[W::template index_of<0>(t, m)]);
    }
    W::forward(x, xc, t, Twiddles(tw_fwd + W::LANE_TABLE_OFFSET, tw_fwd));
    W::forward(y, xc, t, Twiddles(tw_fwd + W::LANE_TABLE_OFFSET, tw_fwd));
#pragma unroll
    for (int m = 0; m < W::E; m++) x[m] = fp_mulmod(fp_mulmod(x[m], fp_center(y[m])), n_inv);
    W::inverse(x, xc, t, Twiddles(tw_inv + W::LANE_TABLE_OFFSET, tw_inv));
#pragma unroll
    for (int m = 0; m < W::E; m++) c[W::template index_of<0>(t, m)] = fp_to_u64(fp_canon(x[m]));
}

// ---------------------------------------------------------------------------------------------
// The rotated read of a step where a wave holds a whole polynomial (PIECES in k_blind_rotate): register m takes word
// ((m + C) mod E) * LANES behind one per-lane LDS byte address, C the same for the whole wave.  One copy of the E reads per C,
// the register offsets as immediates of the reads -- written as instructions: left to the compiler, the copies are merged again
// into one set of reads behind E addresses computed per copy (16 v_add_u32 per step).  The compiler does not count reads it did
// not issue: rotated_reads_landed() waits for them and must follow before w is used.  All E reads are in flight together, where
// the compiler's own schedule waited for each in turn.
template <int BYTES>
__device__ __forceinline__ void rotated_read(double &w, uint32_t from) {
    asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(w) : "v"(from), "n"(BYTES) : "memory");
}
template <int C, int E, int LANES, int... M>
__device__ __forceinline__ void rotated_reads(double (&w)[E], uint32_t from, std::integer_sequence<int, M...>) {
    (rotated_read<((M + C) & (E - 1)) * LANES * 8>(w[M], from), ...);
}
template <int E, int LANES, int... C>
__device__ __forceinline__ void rotated_reads_for(uint32_t c, double (&w)[E], uint32_t from, std::integer_sequence<int, C...>) {
    ((c == (uint32_t)C ? rotated_reads<C, E, LANES>(w, from, std::make_integer_sequence<int, E>{}) : (void)0), ...);
}
template <int E>
__device__ __forceinline__ void rotated_reads_landed(double (&w)[E]) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int m = 0; m < E; m++) asm volatile("" : "+v"(w[m]));   // (nothing reads w[m] before the wait)
}

// ---------------------------------------------------------------------------------------------
// DIG: what the launcher knows about the gadget --
//   0  nothing;
//   1  l <= 5: the 2l lazy products (each below 0.8 q; below 1.2 q after the fused opening of 3) that enter the inverse
//      transform stay below 16 q (its first centring pass is spared);
//   2  also beta <= 9: a balanced digit (|d| <= 2^8) times a twiddle (|w| <= 2^45) is exact in a double;
//   3  also beta <= 7: the first butterfly stage of the forward transforms is two exact FMAs (first_butterfly, fbs_ntt.hpp);
//      where a wave holds a whole polynomial (SplitNtt) the first TWO stages are exact three-term sums (first_two_stages)
//   4  l = 1 (one wide digit, any beta: the shape the 128-bit parameter sets take at N = 2048): as 1, without the loop
//      over further levels -- and without the registers the compiler keeps alive for it
//   5, 6, 7  l = 2 (the 128-bit sets for p <= 4 at N = 1024 and for p = 31, 63): as 1, 2, 3 with the two levels written out
//      (no spills at N = 1024 where the loop form spills 21 registers, 13 instead of 27 at N = 2048)
// FPW: bootstraps per workgroup.  The hardware deals the waves of a workgroup round the four SIMDs of a CU but starts
// every workgroup at the same SIMD often enough that two-wave workgroups pile up on two SIMDs while the other two
// idle whenever a CU holds fewer than four of them (measured: 512 bootstraps took 9.7 ms, 256 took 5.7 ms); four-wave
// workgroups (two bootstraps) always cover all four SIMDs.
// TURNS: the two waves of a SIMD hand the issue priority back and forth (lead_if).  It pays while a launch is a round or two
// long; small workgroups of a long launch are refilled as they finish and do better left alone -- and the mere presence of
// s_setprio costs the compiler's schedule 7 % there (N = 1024, l = 2, 8192 bootstraps: 118 k FBS/s with, 134 k without;
// 1024 bootstraps: 129 against 125), so the launcher picks an instantiation, not a flag.
template <int LOGN, int LL, int DIG, int FPW, bool TURNS = true>
__global__ __launch_bounds__((2 << LL) * FPW) __attribute__((amdgpu_waves_per_eu(2))) void k_blind_rotate(BrArgs a) {
    using W = typename NttFor<LOGN, LL>::type;
    constexpr int FIRST = (DIG == 3 || DIG == 7) ? (has_fused_opening<W>::value ? 3 : 2) : (DIG == 2 || DIG == 6) ? 1 : 0;
    constexpr bool BOUNDED = DIG >= 1;
    constexpr bool ONE_LEVEL = DIG == 4, TWO_LEVELS = DIG >= 5;
#ifndef FBS_PEEL_MAX_LL
#define FBS_PEEL_MAX_LL 6   // measured: peeling costs the two-waves-per-polynomial shapes more in spills than it saves
#endif
    // first level peeled off the loop (it assigns the sums instead of adding to zeros): pays where registers allow
    constexpr bool PEEL = ONE_LEVEL || TWO_LEVELS || LL <= FBS_PEEL_MAX_LL;
    constexpr int N = W::N, E = W::E, LANES = W::LANES;
    // PIECES: a wave holds a whole polynomial, so the rotation X^r of a step splits into a lane part (r mod 64) and a
    // register part (r / 64) that is the same for the whole wave (the step loop below).  Every component's region then
    // starts with a guard slot of LANES words for the lanes whose lane part borrows from the register part.
    constexpr bool PIECES = LL == 6;
    constexpr int GUARD = PIECES ? LANES : 0, REGION = GUARD + 2 * N;
    __shared__ double lds_all[FPW * 2 * REGION];   // [bootstrap][component][guard | ping-pong][N]
    const uint32_t sub = threadIdx.x >> (LL + 1);          // which bootstrap of the workgroup
    const uint32_t comp = __builtin_amdgcn_readfirstlane((threadIdx.x >> LL) & 1u);        // GLWE component owned by this thread: 0 = mask, 1 = body
    const uint32_t t = threadIdx.x & (LANES - 1);
    double *lds = lds_all + sub * (2 * REGION) + GUARD;
    double *mine = lds + comp * REGION;
    double *theirs = lds + (comp ^ 1u) * REGION;
    typename W::Xchg xc{mine, 0};
    Twiddles twf(a.tw_fwd + W::LANE_TABLE_OFFSET, a.tw_fwd), twi(a.tw_inv + W::LANE_TABLE_OFFSET, a.tw_inv);
    if constexpr (LL <= FBS_ONE_BUFFER_MAX_LL) {
        // One exchange buffer per polynomial (fbs_ntt.hpp); the other half of each component's region
        // holds a twiddle table instead (forward in component 0's, inverse in component 1's), so the per-lane
        // twiddle gathers are LDS reads, not 64-address global loads.
        xc.stride = 0;
        double *table = mine + N;
        const double *src = (comp ? a.tw_inv : a.tw_fwd) + W::LANE_TABLE_OFFSET;
#pragma unroll
        for (int m = 0; m < E; m++) table[t + (uint32_t)LANES * m] = src[t + (uint32_t)LANES * m];
        __syncthreads();
        twf.lane = lds + N;
        twi.lane = lds + REGION + N;
    }

    const BrJob job = br_job<N>(a, (size_t)blockIdx.x * FPW + sub);
    const uint32_t *ms = job.ms;
    const uint32_t rows = 2 * a.l;
    double acc[E];
    br_acc_init<N, LANES, 2>(acc, a, job, t, comp != 0u ? 1u : 0u);
    const auto [round_scale, round_offset, sign_bits] = br_rounding(a.l, a.beta);

    const uint32_t t16 = t * 16u;   // this thread's 16 bytes of a register pair's 16 LANES
    uint32_t r_next = ms[0];   // the rotation amount of a step is fetched one step ahead: its latency is never exposed
    constexpr int PRIO = !TURNS ? 0 : LL <= 6 ? FBS_PRIO_ONE_WAVE : FBS_PRIO_MULTI_WAVE;
    const uint32_t slot = PRIO ? wave_slot_parity() : 0u;
    for (uint32_t i = 0; i < a.n; i++) {
        lead_if<PRIO>(PRIO == 7 ? 2u * i : i, slot);
        const uint32_t r = __builtin_amdgcn_readfirstlane(r_next);
        r_next = ms[i + 1];     // ms has n+1 entries; the last one (the body) is read here and ignored
        // X^0 * ACC - ACC = 0: nothing to add (uniform over the two waves of a bootstrap).  Workgroups of several bootstraps run
        // such a step through instead: its digits are all zero, so is every product, and ACC comes out of fp_center unchanged.
        // A skip that still met the other bootstraps' two barriers was a second path into the loop latch, and the compiler
        // carried ACC across it in a second set of registers: 16 v_mov_b64 on every step (one step in 2N takes r = 0).
        if constexpr (FPW == 1)
            if (r == 0) continue;

        // ---- (X^r - 1) * ACC_c, centred, rounded to the closest multiple of q / B^l ---------------
        uint32_t digits[E];
        {
            double *buf = xc.next();
            if constexpr (LL <= FBS_ONE_BUFFER_MAX_LL) W::sync();
            // both the store and the rotated read walk consecutive words across the lanes: no swizzle needed here
#pragma unroll
            for (int m = 0; m < E; m++) buf[t + (uint32_t)LANES * m] = acc[m];
            // Signed representatives, not canonical ones: the rounding below treats q as 2^46, an error proportional
            // to the value -- of one sign on [0, q) (it then adds up coherently through the key bits), symmetric
            // here.  v and acc are centred, so the difference d = v - acc in (-q, q) needs no reduction of its own.
            if constexpr (PIECES) {
                // Coefficient t + 64 m of X^r * ACC is +-ACC[(t + 64 m - r) mod 2N].  With r = 64 rh + rl that is lane
                // t - rl of register m - rh, read mod 2E: bits below E = the register, bit E = the sign -- both the same for
                // every lane of the wave, so they are scalar arithmetic, and a lane supplies ONE address: word t - rl of the
                // buffer.  Lanes t < rl land one register lower (64 words back) by themselves; where that leaves the buffer
                // (register 0 -> register 2E - 1 = minus register E - 1, against the sign of the other lanes) they find the
                // guard slot in front of it, which holds -ACC's last register.  The sign is a factor +-1.0 of the
                // subtraction, one exact FMA in the place of the add: no vector instruction per coefficient for the rotation.
                // (Measured and not kept: +-scale * w + (offset - scale * acc), the second FMA issued under the reads -- the
                // same count, 8.764 against 8.750 ms per launch; profiles/headline_rotation_diet.)
                constexpr int LOGE = LOGN - LL;
                buf[(int)t - LANES] = -acc[E - 1];
                W::sync();
                const uint32_t first = (0u - (r >> LL)) & (uint32_t)(2 * E - 1);   // the register (mod 2E) that register 0 reads
                const uint32_t from = (uint32_t)(uintptr_t)buf + 8u * (t - (r & (uint32_t)(LANES - 1)));   // LDS byte address (in the guard slot where t < rl)
                double w[E];
                rotated_reads_for<E, LANES>(first & (uint32_t)(E - 1), w, from, std::make_integer_sequence<int, E>{});
                rotated_reads_landed(w);
#pragma unroll
                for (int m = 0; m < E; m++) {
                    const double sign = __hiloint2double((int)(0x3FF00000u | (((first + (uint32_t)m) << (31 - LOGE)) & 0x80000000u)), 0);
                    const double d = __builtin_fma(w[m], sign, -acc[m]);
                    digits[m] = (uint32_t)__builtin_fma(d, round_scale, round_offset) ^ sign_bits;   // truncation = floor, < 3 * 2^(l*beta)
                }
            } else {
                W::sync();
                const uint32_t from = (t - r) & (2u * N - 1u);   // coefficient t of X^r * ACC is +-ACC[(t - r) mod 2N]
#pragma unroll
                for (int m = 0; m < E; m++) {
                    const uint32_t idx = from + (uint32_t)LANES * m;   // < 3N: bit LOGN = sign, bits below = position
                    const double w = buf[idx & (N - 1)];
                    const double v = __hiloint2double(__double2hiint(w) ^ (int)((idx << (31 - LOGN)) & 0x80000000u), __double2loint(w));
                    const double d = v - acc[m];
                    digits[m] = (uint32_t)__builtin_fma(d, round_scale, round_offset) ^ sign_bits;   // truncation = floor, < 3 * 2^(l*beta)
                }
            }
        }

        // ---- digits, least significant level first; NTT; multiply-accumulate with the key row ---
        double own[E], other[E];   // contributions to this component and to the partner's (lazy sums)
        // one gadget level; ASSIGN: the first one initialises the sums instead of adding to zeros
        auto level = [&](int lv, auto assign) {
            constexpr bool ASSIGN = decltype(assign)::value;
            const uint32_t shift = ((uint32_t)a.l - 1u - (uint32_t)lv) * a.beta;
            double x[E];
#pragma unroll
            for (int m = 0; m < E; m++)
                x[m] = (double)(int)__builtin_amdgcn_sbfe(digits[m], shift, a.beta);   // balanced digit in [-B/2, B/2)
            // (buffer loads, KeyRows: the step's rows behind one resource, the polynomial picked by a scalar byte offset)
            const KeyRows keys(a.bsk_hat + (size_t)FBS_KEY_STEP(i) * rows * 2 * N);
            const uint32_t krow = ((comp * a.l + (uint32_t)lv) * 2u) * (uint32_t)(N * 8);
            const uint32_t k_own = krow + comp * (uint32_t)(N * 8), k_oth = krow + (comp ^ 1u) * (uint32_t)(N * 8);
            // The first half of the "own" key polynomial is requested before the last butterfly group of the transform
            // (one group ~ one L2 round trip), the rest after it.  Measured on MI355X: 13.5 -> 12.8 ms per 1024-batch;
            // asking for more ahead of time (all of it, or the partner's polynomial too) spills and loses again.
            constexpr int EARLY = E / 4;
            double2 ko[E / 2];
            W::template forward<FIRST>(x, xc, t, twf, [&] {
#pragma unroll
                for (int m = 0; m < EARLY; m++) ko[m] = keys.load(t16 + (uint32_t)(m * LANES * 16), k_own);
            });
#pragma unroll
            for (int m = EARLY; m < E / 2; m++) ko[m] = keys.load(t16 + (uint32_t)(m * LANES * 16), k_own);
            // own products first; each finished pair frees the registers its key words sat in, and the partner's
            // key words are requested into them while the remaining own products run
            double2 kt[E / 2];
#pragma unroll
            for (int j = 0; j < E / 2; j++) {
                const double p0 = fp_mulmod(x[2 * j], ko[j].x), p1 = fp_mulmod(x[2 * j + 1], ko[j].y);
                own[2 * j] = ASSIGN ? p0 : own[2 * j] + p0;
                own[2 * j + 1] = ASSIGN ? p1 : own[2 * j + 1] + p1;
                kt[j] = keys.load(t16 + (uint32_t)(j * LANES * 16), k_oth);
            }
#pragma unroll
            for (int j = 0; j < E / 2; j++) {
                const double p0 = fp_mulmod(x[2 * j], kt[j].x), p1 = fp_mulmod(x[2 * j + 1], kt[j].y);
                other[2 * j] = ASSIGN ? p0 : other[2 * j] + p0;
                other[2 * j + 1] = ASSIGN ? p1 : other[2 * j + 1] + p1;
            }
        };
        if constexpr (TWO_LEVELS) {
            level(1, std::true_type{});
            level(0, std::false_type{});
        } else if constexpr (PEEL) {
            level((int)a.l - 1, std::true_type{});
            if constexpr (!ONE_LEVEL)
                for (int lv = (int)a.l - 2; lv >= 0; lv--) level(lv, std::false_type{});
        } else {
#pragma unroll
            for (int m = 0; m < E; m++) own[m] = other[m] = 0.0;
            for (int lv = (int)a.l - 1; lv >= 0; lv--) level(lv, std::false_type{});
        }

        // ---- hand the partner its half of the external product (same ping-pong slot in both regions) ----
        // (the wave-uniform twiddles of the inverse transform are requested first: scalar loads, in flight across the
        // two barriers instead of in front of the first butterflies)
        const typename W::InvUniform inv_uni = W::inverse_uniform(t, twi);
        {
            const uint32_t slot = xc.pp ? xc.stride : 0;
            xc.pp ^= 1u;
            // one-buffer exchanges: the partner may still be reading its buffer, which is where this hand-off lands
            if constexpr (LL <= FBS_ONE_BUFFER_MAX_LL) __syncthreads();
#pragma unroll
            for (int m = 0; m < E; m++) theirs[slot + W::handoff_word(t, m)] = other[m];
            __syncthreads();
#pragma unroll
            for (int m = 0; m < E; m++) own[m] += mine[slot + W::handoff_word(t, m)];
        }

        if constexpr (PRIO == 7) lead_if<PRIO>(2u * i + 1u, slot);
        // ---- back to coefficients (the 1/N is folded into the key) and accumulate ---------------
        // (a whole polynomial on one wave, inputs below 16 q: the inverse that centres one register per group at the group's exit,
        // 18 centring instructions per step instead of 96 -- same residues, and the same 8 q at the exit)
        if constexpr (has_fused_opening<W>::value && BOUNDED)
            W::inverse_exit_centred(own, xc, t, twi, inv_uni);
        else
            W::template inverse<BOUNDED>(own, xc, t, twi, inv_uni);
#pragma unroll
        for (int m = 0; m < E; m++) acc[m] = fp_center(acc[m] + own[m]);   // |.| <= 17 q -> centred
    }

    if constexpr (FPW == 4) {
        // The benchmark shape keeps br_extract's text written out here.  With the call its step loop has the same 3 284
        // instructions, four FP64 ones in other places (registers 256 -> 252, scratch 20 -> 0 B), and that schedule measured
        // 0.2-0.3 % slower in three jobs (112 252 against 112 597 FBS/s, a second copy of the parent's library 112 551;
        // profiles/rotation_frame).  Written out, the loop's vector instructions are the ones they were.  Every other
        // instantiation takes the call: no slower anywhere it was timed, and 12 to 60 bytes less scratch in most.
        if (!job.live) return;
        if (uint64_t *raw = gate_acc(a.gv, job.f, 2 * N)) {
#pragma unroll
            for (int m = 0; m < E; m++) raw[comp * N + t + (uint32_t)LANES * m] = fp_to_u64(fp_canon(acc[m]));
            return;
        }
        uint64_t *out = gate_out(a.gv, job.f, a.ct_words);
        if (comp == 0) {
#pragma unroll
            for (int m = 0; m < E; m++) {
                const uint32_t j = t + (uint32_t)LANES * m;
                const uint64_t v = fp_to_u64(fp_canon(acc[m]));
                if (j == 0) out[0] = v;
                else out[N - j] = fq_neg(v);
            }
        } else if (t == 0) {
            const uint64_t b = fp_to_u64(fp_canon(acc[0]));
            out[N] = a.post ? fq_add(b, a.post[job.table]) : b;
        }
    } else {
        br_extract<N, LANES, 2>(a, job, acc, comp, t);
    }
}

// ---------------------------------------------------------------------------------------------
// Two key bits per step ("multi-bit" blind rotation, bsk_group = 2).  With E0, E1, E2 the GGSW samples of s0(1-s1),
// (1-s0)s1, s0 s1 for a pair (s0, s1) of key bits and (a0, a1) the pair's rotation amounts,
//     ACC += [ (X^a0 - 1) E0 + (X^a1 - 1) E1 + (X^(a0+a1) - 1) E2 ]  (x)  ACC.
// The bundle in brackets is built in the NTT domain, where X^e - 1 is the pointwise factor zeta^e - 1 (zeta = the
// evaluation point a register holds = psi^(2 bitrev(P) + 1) at array position P; looked up in a table of psi^x - 1), and
// ACC itself is decomposed: no rotate-and-subtract step, no LDS round trip for it, and HALF the transforms per key bit.
// Costs: three key polynomials read and three exact products per key word built (per pair of bits), 1.5x the key, and a
// step's key-noise term triples (params.variances).  Same shapes, layouts and transforms as k_blind_rotate; DIG as there
// (0, 3 and 4 are built).
template <int LOGN, int LL, int DIG>
__global__ __launch_bounds__(2 << LL) __attribute__((amdgpu_waves_per_eu(2))) void k_blind_rotate_pairs(BrArgs a) {
    using W = typename NttFor<LOGN, LL>::type;
    static_assert(W::HAS_EVAL_POSITION, "the bundle needs to know which evaluation point a register holds");
    constexpr int N = W::N, E = W::E, LANES = W::LANES;
    constexpr int FIRST = DIG == 3 ? 2 : 0;
    constexpr bool ONE_LEVEL = DIG == 4;
    // [component][exchange buffer | twiddle table][N], then psi^x for x < N (psi^(x+N) = -psi^x): 5 N words = 40 KB at
    // N = 1024, 80 KB at N = 2048 -- exactly what lets 8 waves share a CU's 160 KB.  The psi table is stored TRANSPOSED,
    // word (x mod G) * N/G + x / G with G = 2^EVAL_GROUP_LOG2: the exponents a wave gathers for one register are G * (e *
    // lane permutation) + uniform, an arithmetic progression of stride G e -- in natural order all 64 lanes of an odd e would
    // fall on 4 of the 32 bank pairs (measured: 2.75e9 conflict cycles per launch, the LDS pipe 66 % busy); transposed they
    // walk the banks with stride e (two-way for odd e, which a 64-lane 8-byte read is anyway; at worst eight-way).
    __shared__ __attribute__((aligned(16384))) double lds_all[2 * 2 * N + N];
    constexpr int GLOG = W::EVAL_GROUP_LOG2, G = 1 << GLOG;
    const uint32_t comp = __builtin_amdgcn_readfirstlane((threadIdx.x >> LL) & 1u);
    const uint32_t t = threadIdx.x & (LANES - 1);
    double *lds = lds_all;
    double *mine = lds + comp * 2 * N;
    double *theirs = lds + (comp ^ 1u) * 2 * N;
    typename W::Xchg xc{mine, 0};
    Twiddles twf(a.tw_fwd + W::LANE_TABLE_OFFSET, a.tw_fwd), twi(a.tw_inv + W::LANE_TABLE_OFFSET, a.tw_inv);
    static_assert(LL <= FBS_ONE_BUFFER_MAX_LL, "one exchange buffer per polynomial, twiddle tables beside it");
    {
        xc.stride = 0;
        double *table = mine + N;
        const double *src = (comp ? a.tw_inv : a.tw_fwd) + W::LANE_TABLE_OFFSET;
#pragma unroll
        for (int m = 0; m < E; m++) table[t + (uint32_t)LANES * m] = src[t + (uint32_t)LANES * m];
#pragma unroll
        for (int m = 0; m < E / 2; m++) {   // the two components' threads copy half of the psi table each
            const uint32_t x = comp * (N / 2) + t + (uint32_t)LANES * m;
            lds[4 * N + (x & (G - 1)) * (N / G) + (x >> GLOG)] = a.psi_pow[x];
        }
        __syncthreads();
        twf.lane = lds + N;
        twi.lane = lds + 3 * N;
    }

    const BrJob job = br_job<N>(a, blockIdx.x);
    const uint32_t *ms = job.ms;
    const uint32_t rows = 2 * a.l;
    double acc[E];
    br_acc_init<N, LANES, 2>(acc, a, job, t, comp != 0u ? 1u : 0u);
    const auto [round_scale, round_offset, sign_bits] = br_rounding(a.l, a.beta);
    // zeta^e for the evaluation point zeta = psi^o a register holds: exponent x = e * o mod 2N, o = o_lane + c_m with
    // o_lane = 2 bitrev(lane part of the array position) + 1 = G k_lane + r_lane (r_lane wave-uniform) and c_m = 2 bitrev(
    // register part), a compile-time constant.  x = G a + b with b wave-uniform; table word b N/G + (a mod N/G), sign = bit
    // log2(N/G) of a.  Everything but e * k_lane is scalar arithmetic.
    const uint32_t o_lane = 2u * (__builtin_bitreverse32(W::eval_position_lane(t)) >> (32 - LOGN)) + 1u;
    const uint32_t k_lane8 = (o_lane >> GLOG) << 3;
    const uint32_t r_lane = __builtin_amdgcn_readfirstlane(o_lane & (G - 1));
    constexpr uint32_t MASK8 = (uint32_t)(N / G - 1) << 3;
    const uint32_t psi_base = (uint32_t)(uintptr_t)(lds + 4 * N);   // LDS byte address of the table (16 KB aligned)

    const uint32_t t16 = t * 16u;   // this thread's 16 bytes of a register pair's 16 LANES
    const uint32_t n_pairs = a.n / 2;
    uint32_t e0_next = ms[0], e1_next = ms[1];
    constexpr int PRIO = LL <= 6 ? FBS_PRIO_ONE_WAVE : FBS_PRIO_MULTI_WAVE;
    const uint32_t slot = PRIO ? wave_slot_parity() : 0u;
    for (uint32_t i = 0; i < n_pairs; i++) {
        lead_if<PRIO>(PRIO == 7 ? 2u * i : i, slot);
        uint32_t e[3];
        e[0] = __builtin_amdgcn_readfirstlane(e0_next);
        e[1] = __builtin_amdgcn_readfirstlane(e1_next);
        e0_next = ms[2 * i + 2 < a.n ? 2 * i + 2 : a.n];   // (the last pair re-reads the body word and ignores it)
        e1_next = ms[2 * i + 3 < a.n ? 2 * i + 3 : a.n];
        if (e[0] == 0 && e[1] == 0) continue;               // the bundle is zero (uniform over the bootstrap's waves)
        e[2] = (e[0] + e[1]) & (2u * N - 1u);
        uint32_t lane8[3];
#pragma unroll
        for (int jj = 0; jj < 3; jj++) lane8[jj] = __umul24(e[jj], k_lane8);

        // ---- ACC_c itself, rounded to the closest multiple of q / B^l; packed balanced digits -------------
        uint32_t digits[E];
#pragma unroll
        for (int m = 0; m < E; m++) digits[m] = (uint32_t)__builtin_fma(acc[m], round_scale, round_offset) ^ sign_bits;

        double own[E], other[E];
        auto level = [&](int lv, auto assign) {
            constexpr bool ASSIGN = decltype(assign)::value;
            const uint32_t shift = ((uint32_t)a.l - 1u - (uint32_t)lv) * a.beta;
            double x[E];
#pragma unroll
            for (int m = 0; m < E; m++) x[m] = (double)(int)__builtin_amdgcn_sbfe(digits[m], shift, a.beta);
            // (the exponents are "redefined" here so that the 48 uniform products e * c_m below are computed where they are
            // used, level by level, instead of being hoisted out of the level loop into more SGPRs than there are)
            uint32_t e_lv[3] = {e[0], e[1], e[2]};
            if constexpr (!ONE_LEVEL) asm volatile("" : "+s"(e_lv[0]), "+s"(e_lv[1]), "+s"(e_lv[2]));
            // the step's key rows (three samples of `rows` rows of two polynomials) behind one buffer resource; own / partner's
            // polynomial of this component's row of sample jj: scalar byte offsets
            const KeyRows keys(a.bsk_hat + (size_t)FBS_KEY_STEP(i) * 3 * rows * 2 * N);
            uint32_t k_own[3], k_oth[3];
#pragma unroll
            for (int jj = 0; jj < 3; jj++) {
                const uint32_t krow = (((uint32_t)jj * rows + comp * a.l + (uint32_t)lv) * 2u) * (uint32_t)(N * 8);
                k_own[jj] = krow + comp * (uint32_t)(N * 8);
                k_oth[jj] = krow + (comp ^ 1u) * (uint32_t)(N * 8);
            }
            // what one register pair (2j, 2j+1) needs from memory: its words of the six key polynomials ...
            struct PairKeys {
                double2 ko[3], kt[3];
            };
            auto request = [&](auto jc, PairKeys &in) {
                constexpr int j = decltype(jc)::value;
#pragma unroll
                for (int jj = 0; jj < 3; jj++) {
                    in.ko[jj] = keys.load(t16 + (uint32_t)(j * LANES * 16), k_own[jj]);
                    in.kt[jj] = keys.load(t16 + (uint32_t)(j * LANES * 16), k_oth[jj]);
                }
            };
            auto consume = [&](auto jc, const PairKeys &in) {
                constexpr int j = decltype(jc)::value;
                // ... and zeta^e - 1 for its two registers and the three exponents, from the table of psi^x in LDS
                // One look-up per exponent serves BOTH registers of the pair: 2j and 2j + 1 differ in bit 0 of their array position,
                // i.e. in the top bit of its reversal, so their evaluation points differ by psi^N = -1 and zeta_(2j+1)^e = (-1)^e
                // zeta_(2j)^e -- a wave-uniform sign (round 3: half the gathers from the table, and half their bank conflicts).
                static_assert(W::eval_position_reg(1) - W::eval_position_reg(0) == 1, "registers 2j, 2j+1 hold neighbouring array positions");
                double mono[3][2];
#pragma unroll
                for (int jj = 0; jj < 3; jj++) {
                    const uint32_t c_m = 2u * (__builtin_bitreverse32(W::eval_position_reg(2 * j)) >> (32 - LOGN));
                    const uint32_t rsum = r_lane + (c_m & (G - 1));                       // uniform from here ...
                    const uint32_t ku = (c_m >> GLOG) + (rsum >> GLOG), ru = rsum & (G - 1);
                    const uint32_t eru = e_lv[jj] * ru;
                    const uint32_t u8 = (e_lv[jj] * ku + (eru >> GLOG)) << 3;
                    const uint32_t sbase = psi_base + (eru & (G - 1)) * (uint32_t)(N / G * 8);
                    const uint32_t odd = e_lv[jj] << 31;                                   // ... to here
                    const uint32_t t8 = lane8[jj] + u8;
                    const double v = *reinterpret_cast<const __attribute__((address_space(3))) double *>((t8 & MASK8) | sbase);
                    // (+-) by the bit above the table index, then - 1
                    const int hi = __double2hiint(v) ^ (int)((t8 << (31 - 3 - (LOGN - GLOG))) & 0x80000000u);
                    mono[jj][0] = __hiloint2double(hi, __double2loint(v)) - 1.0;
                    mono[jj][1] = __hiloint2double(hi ^ (int)odd, __double2loint(v)) - 1.0;
                }
                // key words of the bundle: lazy sums of three exact products (< 2.3 q).  With |x| < 2^49.3 (general first
                // stage) the product below stays within 0.9 q as it is; the two-FMA first stage leaves |x| near 2^51 and
                // wants the word centred first.
                // (the first product initialises the sums: 0.0 + x is an instruction the compiler may not drop, -0.0 being a double)
                double wo0 = fp_mulmod(in.ko[0].x, mono[0][0]), wo1 = fp_mulmod(in.ko[0].y, mono[0][1]);
                double wt0 = fp_mulmod(in.kt[0].x, mono[0][0]), wt1 = fp_mulmod(in.kt[0].y, mono[0][1]);
#pragma unroll
                for (int jj = 1; jj < 3; jj++) {
                    wo0 += fp_mulmod(in.ko[jj].x, mono[jj][0]);
                    wo1 += fp_mulmod(in.ko[jj].y, mono[jj][1]);
                    wt0 += fp_mulmod(in.kt[jj].x, mono[jj][0]);
                    wt1 += fp_mulmod(in.kt[jj].y, mono[jj][1]);
                }
                if constexpr (FIRST == 2) {
                    wo0 = fp_center(wo0);
                    wo1 = fp_center(wo1);
                    wt0 = fp_center(wt0);
                    wt1 = fp_center(wt1);
                }
                const double p0 = fp_mulmod(x[2 * j], wo0), p1 = fp_mulmod(x[2 * j + 1], wo1);
                const double r0 = fp_mulmod(x[2 * j], wt0), r1 = fp_mulmod(x[2 * j + 1], wt1);
                own[2 * j] = ASSIGN ? p0 : own[2 * j] + p0;
                own[2 * j + 1] = ASSIGN ? p1 : own[2 * j + 1] + p1;
                other[2 * j] = ASSIGN ? r0 : other[2 * j] + r0;
                other[2 * j + 1] = ASSIGN ? r1 : other[2 * j + 1] + r1;
            };
            // The key words of pair 0 are requested before the last butterfly group of the transform, those of pair j right
            // before it is consumed (keeping pair j+1 in flight as well was measured: 35 registers spilled, no gain).
            PairKeys in;
            W::template forward<FIRST>(x, xc, t, twf, [&] { request(std::integral_constant<int, 0>{}, in); });
            static_assert(E == 16, "eight register pairs, written out");
            // (round 3, with the buffer loads' forty spare registers: pair j + 1 requested before pair j is consumed -- 9.21 against 9.23 ms
            // per 1024 bootstraps at the 128-bit p = 15 set, i.e. nothing: left as it was)
#define FBS_PAIR_STEP(J)                                                                                    \
    if constexpr ((J) > 0) request(std::integral_constant<int, (J)>{}, in);                                 \
    consume(std::integral_constant<int, (J)>{}, in);                                                        \
    if constexpr (!ONE_LEVEL) __builtin_amdgcn_sched_barrier(0);
            FBS_PAIR_STEP(0) FBS_PAIR_STEP(1) FBS_PAIR_STEP(2) FBS_PAIR_STEP(3)
            FBS_PAIR_STEP(4) FBS_PAIR_STEP(5) FBS_PAIR_STEP(6) FBS_PAIR_STEP(7)
#undef FBS_PAIR_STEP
        };
        level((int)a.l - 1, std::true_type{});
        if constexpr (!ONE_LEVEL)
            for (int lv = (int)a.l - 2; lv >= 0; lv--) level(lv, std::false_type{});

        // ---- hand the partner its half, inverse transform, accumulate: as in k_blind_rotate ---------------
        const typename W::InvUniform inv_uni = W::inverse_uniform(t, twi);
        {
            __syncthreads();
#pragma unroll
            for (int m = 0; m < E; m++) theirs[W::handoff_word(t, m)] = other[m];
            __syncthreads();
#pragma unroll
            for (int m = 0; m < E; m++) own[m] += mine[W::handoff_word(t, m)];
        }
        if constexpr (PRIO == 7) lead_if<PRIO>(2u * i + 1u, slot);
        W::template inverse<true>(own, xc, t, twi, inv_uni);   // 2l products below 0.8 q each: l <= 5 (the launcher checks)
#pragma unroll
        for (int m = 0; m < E; m++) acc[m] = fp_center(acc[m] + own[m]);
    }

    br_extract<N, LANES, 2>(a, job, acc, comp, t);
}

// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------
#define FBS_FOR_EACH_SHAPE(X) X(8) X(9) X(10) X(11) X(12)

// d_given: the key in the coefficient domain, already on the device (keys made there, fbs_keygen.hip); null: ctx->bsk is uploaded
template <int LOGN>
static int transform_bsk_t(fbs_ctx *ctx, const uint64_t *d_given) {
    constexpr int LL = lanes_log2_for(LOGN);
    const fbs_params &p = ctx->p;
    const uint32_t N = ctx->N;
    const size_t polys = ctx->n_ggsw * ctx->rows * (p.k + 1);
    uint64_t *d_own = nullptr;
    hipError_t e = hipSuccess;
    if (!d_given) {
        FBS_HIP(ctx, hipMalloc(&d_own, polys * N * 8));
        e = hipMemcpyAsync(d_own, ctx->bsk.data(), polys * N * 8, hipMemcpyHostToDevice, ctx->stream);
        ctx->bsk_upload_bytes = (int64_t)(polys * N * 8);
    }
    const uint64_t *d_src = d_given ? d_given : d_own;
    if (e == hipSuccess) {
        const double n_inv = fq_centered(fq_inv(N));
        unsigned grid = (unsigned)std::min<size_t>(polys, 4096);
        hipLaunchKernelGGL((k_key_transform<LOGN, LL, KeyWords>), dim3(grid), dim3(1 << LL), 0, ctx->stream, KeyWords{d_src},
                           reinterpret_cast<double *>(ctx->d_bsk_hat), reinterpret_cast<const double *>(ctx->d_tw_fwd), n_inv,
                           polys);
        e = hipGetLastError();
        constexpr int LLS = lanes_log2_for_small_launch(LOGN);
        if (small_key_needed(ctx)) {
            if (e == hipSuccess && !ctx->d_bsk_hat_small) e = hipMalloc(&ctx->d_bsk_hat_small, polys * N * 8);
            if (e == hipSuccess) {
                hipLaunchKernelGGL((k_key_transform<LOGN, LLS, KeyWords>), dim3(grid), dim3(1 << LLS), 0, ctx->stream, KeyWords{d_src},
                                   reinterpret_cast<double *>(ctx->d_bsk_hat_small), reinterpret_cast<const double *>(ctx->d_tw_fwd),
                                   n_inv, polys);
                e = hipGetLastError();
            }
        }
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (d_own) (void)hipFree(d_own);
    if (e != hipSuccess) return set_error(ctx, FBS_E_DEVICE, std::string("bootstrapping-key transform: ") + hipGetErrorString(e));
    return FBS_OK;
}

int dev_transform_bsk(fbs_ctx *ctx, const uint64_t *d_src) {
    switch (ctx->p.log_n_poly) {
#define X(L) case L: return transform_bsk_t<L>(ctx, d_src);
        FBS_FOR_EACH_SHAPE(X)
#undef X
    }
    return set_error(ctx, FBS_E_INVALID, "unsupported N");
}

// the twiddle tables (and psi^x for two key bits per step), and on first use the device buffers of both keys
int dev_upload_tables(fbs_ctx *ctx) {
    const fbs_params &p = ctx->p;
    const uint32_t N = ctx->N;
    std::vector<uint64_t> fwd, inv;
    host_twiddles(p.log_n_poly, fwd, inv);
    // the table, its two half-size and four quarter-size subtrees, the fused opening's two products (tw_table_words)
    std::vector<double> fwd_c(tw_table_words(N)), inv_c(tw_table_words(N));
    for (uint32_t i = 0; i < tw_table_words(N); i++) {
        fwd_c[i] = fq_centered(fwd[i]);
        inv_c[i] = fq_centered(inv[i]);
    }
    const size_t bsk_words = ctx->n_ggsw * ctx->rows * (p.k + 1) * N;
    const size_t ksk_rows = (size_t)ctx->D * p.t_ksk;
    if (!ctx->d_tw_fwd) {
        FBS_HIP(ctx, hipMalloc(&ctx->d_tw_fwd, (size_t)tw_table_words(N) * 8));
        FBS_HIP(ctx, hipMalloc(&ctx->d_tw_inv, (size_t)tw_table_words(N) * 8));
        FBS_HIP(ctx, hipMalloc(&ctx->d_bsk_hat, bsk_words * 8));
        FBS_HIP(ctx, hipMalloc(&ctx->d_ksk, ksk_rows * ctx->ksk_stride * 8));
        FBS_HIP(ctx, hipMalloc(&ctx->d_ksk_f, ksk_rows * ctx->ksk_stride * 8));
        FBS_HIP(ctx, hipMalloc(&ctx->d_ks_corr, (size_t)ctx->ksk_stride * 8));
    }
    FBS_HIP(ctx, hipMemcpyAsync(ctx->d_tw_fwd, fwd_c.data(), fwd_c.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    FBS_HIP(ctx, hipMemcpyAsync(ctx->d_tw_inv, inv_c.data(), inv_c.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    if (ctx->group == 2) {   // psi^x, x < N: what the pointwise factors zeta^e - 1 of the monomials X^e - 1 are made from
        std::vector<double> tbl(N);
        const uint64_t psi = fq_pow(FQ_GENERATOR, (FQ - 1) / (2ull * N));
        uint64_t pw = 1;
        for (uint32_t x = 0; x < N; x++) {
            tbl[x] = fq_centered(pw);
            pw = fq_mul(pw, psi);
        }
        if (!ctx->d_psi_pow) FBS_HIP(ctx, hipMalloc(&ctx->d_psi_pow, tbl.size() * 8));
        FBS_HIP(ctx, hipMemcpy(ctx->d_psi_pow, tbl.data(), tbl.size() * 8, hipMemcpyHostToDevice));
    }
    FBS_HIP(ctx, hipStreamSynchronize(ctx->stream));   // fwd_c / inv_c are about to go out of scope
    return FBS_OK;
}

// the key-switching key from ctx->ksk: padded rows, centred doubles, the correction row, the GEMM's limb fragments
int dev_upload_ksk(fbs_ctx *ctx) {
    const fbs_params &p = ctx->p;
    const size_t ksk_rows = (size_t)ctx->D * p.t_ksk;
    // (B/2) * sum of all key rows: what turns the unsigned bit fields of the key-switch kernels into balanced digits
    std::vector<uint64_t> corr(ctx->ksk_stride, 0);
    {
        std::vector<unsigned __int128> sum(p.n + 1, 0);
        for (size_t r = 0; r < ksk_rows; r++)
            for (uint32_t i = 0; i <= p.n; i++) sum[i] += ctx->ksk[r * (p.n + 1) + i];
        for (uint32_t i = 0; i <= p.n; i++) corr[i] = fq_mul((uint64_t)(sum[i] % FQ), 1ull << (p.gamma_ksk - 1));
    }
    FBS_HIP(ctx, hipMemcpyAsync(ctx->d_ks_corr, corr.data(), corr.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    FBS_HIP(ctx, hipMemsetAsync(ctx->d_ksk, 0, ksk_rows * ctx->ksk_stride * 8, ctx->stream));
    FBS_HIP(ctx, hipMemcpy2DAsync(ctx->d_ksk, (size_t)ctx->ksk_stride * 8, ctx->ksk.data(), (size_t)(p.n + 1) * 8,
                                  (size_t)(p.n + 1) * 8, ksk_rows, hipMemcpyHostToDevice, ctx->stream));
    {   // centred doubles for the FP64 key-switch kernel, padded like the integer copy
        std::vector<double> kf(ksk_rows * (size_t)ctx->ksk_stride, 0.0);
        for (size_t r = 0; r < ksk_rows; r++)
            for (uint32_t i = 0; i <= p.n; i++) kf[r * ctx->ksk_stride + i] = fq_centered(ctx->ksk[r * (p.n + 1) + i]);
        FBS_HIP(ctx, hipMemcpy(ctx->d_ksk_f, kf.data(), kf.size() * 8, hipMemcpyHostToDevice));
    }
    FBS_HIP(ctx, hipStreamSynchronize(ctx->stream));   // corr is about to go out of scope
    return dev_keyswitch_gemm_setup(ctx);
}

int dev_upload_keys(fbs_ctx *ctx) {
    if (int rc = dev_upload_tables(ctx)) return rc;
    if (int rc = dev_upload_ksk(ctx)) return rc;
    return dev_transform_bsk(ctx, nullptr);
}

// the instantiation of a k_blind_rotate or k_blind_rotate_pairs descriptor (fbs_select.hpp); false for any other
static bool launch_blind_rotate_main(const Kernel &k, const BrArgs &a, hipStream_t stream) {
    if (k.family == Family::BLIND_ROTATE) {
#define X(L, LL, DIG, FPW, TURNS)                                                                                               \
    if (k.t[0] == L && k.t[1] == (LL) && k.t[2] == DIG && k.t[3] == FPW && k.alt == !(TURNS)) {                                 \
        hipLaunchKernelGGL((k_blind_rotate<L, LL, DIG, FPW, TURNS>), dim3((unsigned)((a.count + FPW - 1) / FPW)),              \
                           dim3((2 << (LL)) * FPW), 0, stream, a);                                                              \
        return true;                                                                                                            \
    }
        FBS_BR_KERNELS(X)
#undef X
    }
    if (k.family == Family::PAIRS) {
#define X(L, DIG)                                                                                                               \
    if (k.t[0] == L && k.t[1] == lanes_log2_for(L) && k.t[2] == DIG) {                                                          \
        hipLaunchKernelGGL((k_blind_rotate_pairs<L, lanes_log2_for(L), DIG>), dim3((unsigned)a.count), dim3(2 << lanes_log2_for(L)), \
                           0, stream, a);                                                                                       \
        return true;                                                                                                            \
    }
        FBS_PAIRS_KERNELS(X)
#undef X
    }
    return false;
}

int dev_blind_rotate(fbs_ctx *ctx, const fbs_tvset *tv, const GateView &gv, const uint32_t *d_ms, hipStream_t stream,
                     const BrStart *start) {
    const fbs_params &p = ctx->p;
    BrArgs a{};
    if (start) {
        // a fused rotation leaves its whole accumulator for several tables to extract from: that has no meaning for a table that
        // is itself the accumulator.  One caller wants the rotated sample itself (encrypted tables, fbs_rotate_dev): it names rows of
        // whole accumulators and a dst_slot whose entries carry the accumulator bit, and nothing of a fused program
        if (start->whole) {
            if (gv.acc_rows || !gv.out_rows || !gv.dst_slot || gv.row_words != (p.k + 1) * ctx->N)
                return set_error(ctx, FBS_E_INVALID, "a rotated sample goes into rows of (k + 1) N words");
        } else if (gv.acc_rows || gv.row_words) {
            return set_error(ctx, FBS_E_INVALID, "a rotation of an encrypted table cannot be a fused one");
        }
        if (!start->d_acc0 || start->n_acc == 0) return set_error(ctx, FBS_E_INVALID, "no encrypted table to rotate");
        a.acc0 = start->d_acc0;
        a.n_acc = start->n_acc;
        a.acc_of = start->d_acc_of;
    } else if (!tv) {
        return set_error(ctx, FBS_E_INVALID, "null argument");
    }
    a.ms = d_ms;
    a.tw_fwd = reinterpret_cast<const double *>(ctx->d_tw_fwd);
    a.tw_inv = reinterpret_cast<const double *>(ctx->d_tw_inv);
    a.psi_pow = reinterpret_cast<const double *>(ctx->d_psi_pow);
    a.tvs = tv ? tv->d_tvs : nullptr;   // (never read where the rotation starts from an encrypted table)
    a.post = tv && !start ? tv->d_post : nullptr;   // br_extract adds a constant where it has one: none with an encrypted table
    a.n = p.n;
    a.l = p.l_bsk;
    a.beta = p.beta_bsk;
    a.ct_words = ctx->D + 1;
    // (entry n_tables of the set is TV_0: selectable only by the rotations of a fused program, whose ids the host wrote)
    a.n_tables = !tv ? 1u : (gv.acc_rows || gv.row_words) ? tv->n_tables + 1 : std::max(1u, tv->n_tables);
    if (gv.count > 0x7FFFFFFFull) return set_error(ctx, FBS_E_INVALID, "batch too large for one launch");
    for (const Launch &l : select_blind_rotate(ctx, gv.count)) {
        a.gv = gv;
        a.gv.f_begin += l.first;
        a.gv.count = a.count = l.count;
        a.acc_first = (uint32_t)((start ? start->first : 0) + l.first);
        if (a.gv.out_rows) a.gv.out_rows += l.first * (size_t)(gv.row_words ? gv.row_words : ctx->D + 1);
        a.bsk_hat = reinterpret_cast<const double *>(reads_small_key(l.kernel) ? ctx->d_bsk_hat_small : ctx->d_bsk_hat);
        ctx->prof.kernel[1] = kernel_name(l.kernel);
        hipEvent_t e0, e1;
        prof_begin(ctx, 1, stream, &e0, &e1);
        if (!launch_blind_rotate_main(l.kernel, a, stream) && !launch_blind_rotate_cu(l.kernel, a, stream) &&
            !launch_blind_rotate_k2(l.kernel, a, stream) && !launch_blind_rotate_glwe(l.kernel, a, stream)) {
            if (e0) ctx->prof.pool.push_back({e0, e1});   // (the event pair goes back: nothing was recorded between them)
            return set_error(ctx, FBS_E_INVALID, "no instantiation of " + ctx->prof.kernel[1]);
        }
        prof_end(ctx, 1, stream, e0, e1);
        FBS_HIP(ctx, hipGetLastError());
    }
    return FBS_OK;
}

int dev_polymul(fbs_ctx *ctx, const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_c, hipStream_t stream) {
    const double n_inv = fq_centered(fq_inv(ctx->N));
    const double *twf = reinterpret_cast<const double *>(ctx->d_tw_fwd), *twi = reinterpret_cast<const double *>(ctx->d_tw_inv);
    switch (ctx->p.log_n_poly) {
#define X(L)                                                                                                               \
    case L:                                                                                                                \
        hipLaunchKernelGGL((k_polymul<L, lanes_log2_for(L)>), dim3(1), dim3(1 << lanes_log2_for(L)), 0, stream, d_a, d_b, \
                           d_c, twf, twi, n_inv);                                                                          \
        break;
        FBS_FOR_EACH_SHAPE(X)
#undef X
        default: return set_error(ctx, FBS_E_INVALID, "unsupported N");
    }
    FBS_HIP(ctx, hipGetLastError());
    return FBS_OK;
}

}  // namespace fbs

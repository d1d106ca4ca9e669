// What the blind-rotation kernels of fbs_blind_rotate.hip, fbs_blind_rotate_cu.hip, fbs_blind_rotate_k2.hip and
// fbs_blind_rotate_glwe.hip share: launch arguments, the issue-priority hand-over of the two waves of a SIMD, key words through
// buffer loads, the frame of a kernel (which bootstrap a thread works on, the initial accumulator, the rounding constants, sample
// extraction) and the launchers of the other three files; and the one-time transform of a key (k_key_transform), which
// fbs_pack.hip and fbs_keygen.hip launch too.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "fbs_gate.hpp"
#include "fbs_internal.hpp"
#include "fbs_ntt.hpp"
#include "fbs_ntt_split.hpp"

namespace fbs {

struct BrArgs {
    GateView gv;
    const uint32_t *ms;      // [count][n+1], values in [0, 2N)
    const double *bsk_hat;   // [n][rows][2][N]  centred, NTT order, times 1/N
    const double *tw_fwd, *tw_inv;
    const uint64_t *tvs;     // [tables][N]
    const uint64_t *post;    // [tables]; null exactly when acc0 is set: sample extraction then adds no constant
    uint32_t n, l, beta, ct_words, n_tables;
    size_t count;            // bootstraps in this launch
    const double *psi_pow;   // [N] psi^x, centred (two key bits per step only)
    // encrypted-index reads (include/fbs_exec.h): the rotation starts from a whole GLWE sample instead of (0, .., 0, TV)
    const uint64_t *acc0;    // [n_acc][(k + 1) N] canonical residues; null: the trivial sample, every kernel as it always was
    const uint32_t *acc_of;  // [bootstraps of the CALL] which sample each starts from; null: bootstrap i of the call from sample i
    uint32_t n_acc;
    uint32_t acc_first;      // the launch's first bootstrap, counted within the call (a call may be cut into several launches)
};

// Issue priority of the two waves that share a SIMD.  They sit in wave slots 0 and 1 of it (HW_ID bits 3:0); left alone,
// the SIMD issues the older one first whenever both are ready.  PRIO = 1: the priority is raised on even steps in one slot
// and on odd steps in the other; PRIO = 7: it also changes hands in the middle of a step (before the inverse transform), so
// that within each half of a step one wave leads and the other fills its stalls, and neither leads for long.
// Measured (tools/selector_bench.py, one box, FBS/s without / PRIO 1 / PRIO 7): N = 1024 one polynomial per wave: p = 2
// 148.3 / 153.0 / 155.0 k, p = 4 125.0 / 126.8 / 129.7 k, and the benchmark shape in whole-CU workgroups 100.0 / 106.8 /
// 110.0 k; N = 2048 (two waves per polynomial): (15, 70) 100.1 / 101.0 / 36 k, (31, 325) 46.3 / 46.8 / 24 k -- a change of
// hands between the barriers of a multi-wave transform stalls the polynomial's other wave.
#ifndef FBS_PRIO_ONE_WAVE
#define FBS_PRIO_ONE_WAVE 7    // polynomials that live in one wave (N <= 1024)
#endif
#ifndef FBS_PRIO_MULTI_WAVE
#define FBS_PRIO_MULTI_WAVE 1  // polynomials spread over several waves
#endif
__device__ __forceinline__ uint32_t wave_slot_parity() {
    uint32_t hw_id;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_id));
    return hw_id & 1u;
}
template <int PRIO>
__device__ __forceinline__ void lead_if(uint32_t turn, uint32_t slot) {
    if constexpr (PRIO != 0) {
        if ((turn ^ slot) & 1u) __builtin_amdgcn_s_setprio(1);
        else __builtin_amdgcn_s_setprio(0);
    }
}

// Key words through BUFFER loads.  The resource (base address of the step's key rows, four SGPRs) and the distance to the
// polynomial wanted (one SGPR) are wave-uniform; every thread supplies ONE 32-bit byte offset, and register pairs further along the
// polynomial are reached through the instruction's immediate offset -- no 64-bit address arithmetic on the vector pipe and no
// register pair per address (flat global loads: 78 of the 2 873 vector instructions of a k_blind_rotate_pairs<11,7,4> step and
// more than thirty registers went into addresses).  `base` must be wave-uniform.
// -DFBS_EXP_HOT_KEYS=1 (experiments only: WRONG results): every step reads the key rows of step 0 or 1, which stay in L2 -- what a
// launch would take if no key word ever came from further away than L2
#ifndef FBS_EXP_HOT_KEYS
#define FBS_EXP_HOT_KEYS 0
#endif
#define FBS_KEY_STEP(i) (FBS_EXP_HOT_KEYS ? ((i) & 1u) : (i))
struct KeyRows {
    __amdgpu_buffer_rsrc_t rsrc;
    __device__ __forceinline__ explicit KeyRows(const double *base)
        : rsrc(__builtin_amdgcn_make_buffer_rsrc(const_cast<double *>(base), 0, 0x7FFFFFFF, 0x00020000)) {}
    // 16 bytes at base + poly_bytes + thread_bytes (+ the immediate the compiler splits off thread_bytes' constant part)
    __device__ __forceinline__ double2 load(uint32_t thread_bytes, uint32_t poly_bytes) const {
        typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, thread_bytes, poly_bytes, 0);
        double2 r;
        r.x = __hiloint2double((int)v.y, (int)v.x);
        r.y = __hiloint2double((int)v.w, (int)v.z);
        return r;
    }
};

// ---------------------------------------------------------------------------------------------
// The frame of a blind-rotation kernel: everything around its step loop.  Every kernel opens with br_job, br_acc_init and
// br_rounding and closes with br_extract; what lies between (LDS, twiddles, key addressing, the steps) is the kernel's own.

// Which bootstrap a thread works on.  f_want: the bootstrap of the launch its workgroup (and, with several bootstraps per
// workgroup, its part of the workgroup) stands for.  One past the end of a ragged batch repeats the last bootstrap -- its waves
// must keep meeting the others at the barriers -- and is not `live`: br_extract writes nothing for it.
struct BrJob {
    bool live;
    size_t f;             // bootstrap of the launch, < a.count
    uint32_t table;       // its table, < a.n_tables
    const uint32_t *ms;   // its n + 1 rotation amounts, the body's last
    const uint64_t *tv;   // its table's test polynomial
};
template <int N>
__device__ __forceinline__ BrJob br_job(const BrArgs &a, size_t f_want) {
    BrJob job;
    job.live = f_want < a.count;
    job.f = job.live ? f_want : a.count - 1;
    size_t gate, ms_row;
    gate_of(a.gv, job.f, &gate, &ms_row);
    // ids that arrive in device memory cannot be validated by the host: an id past the set reads table 0, never past
    // the end of the buffer
    job.table = a.gv.table_ids ? a.gv.table_ids[gate] : 0;
    if (job.table >= a.n_tables) job.table = 0;
    job.ms = a.ms + ms_row * (a.n + 1);
    job.tv = a.tvs + (size_t)job.table * N;
    return job;
}

// ACC = (0, .., 0, X^{-b~} * TV), kept CENTRED (|.| <= (q-1)/2) for the whole rotation; register m of thread t of a component
// is coefficient t + LANES * m.  `comp` (wave-uniform): the component this thread holds, the body being component K1 - 1.
// With a.acc0 set (encrypted-index reads) ACC = X^{-b~} * (the GLWE sample the bootstrap starts from): every component makes the
// gather the body makes from the test polynomial, from its own polynomial of the sample.  One wave-uniform branch on a kernel
// argument, taken once per bootstrap; a sample id that arrived in device memory and lies past the set reads sample 0.
template <int N, int LANES, int K1, int E>
__device__ __forceinline__ void br_acc_init(double (&acc)[E], const BrArgs &a, const BrJob &job, uint32_t t, uint32_t comp) {
    const uint32_t r = (2u * N - job.ms[a.n]) & (2u * N - 1u);
    const bool body = comp == (uint32_t)(K1 - 1);
    // one gather for both: what differs is where it reads and whether a mask component keeps what it read (written as two
    // loops behind a branch, nine kernels took more registers; as one, none does: profiles/lookup/resources.txt)
    const uint64_t *src = job.tv;
    bool mine = body;
    if (a.acc0) {
        const size_t i = (size_t)a.acc_first + job.f;
        uint32_t id = a.acc_of ? a.acc_of[i] : (uint32_t)i;
        if (id >= a.n_acc) id = 0;
        src = a.acc0 + ((size_t)id * K1 + comp) * N;
        mine = true;
    }
#pragma unroll
    for (int m = 0; m < E; m++) {
        const uint32_t idx = (t + (uint32_t)LANES * m - r) & (2u * N - 1u);
        const uint64_t v = src[idx & (N - 1)];
        acc[m] = mine ? fp_center(fp_from_u64((idx & N) ? fq_neg(v) : v)) : 0.0;
    }
}

// Rounding runs on doubles too (floor(x * 2^-s + c) is exact on integers): abar = (d + 2^(s-1)) >> s with
// s = 46 - l*beta, d = what a step decomposes (a centred residue, or the difference of two: an integer in (-q, q), not reduced
// again), abar kept mod B^l -- B^l is added so that the value converted to an unsigned word is positive (l*beta <= 30).  Adding
// B/2 at every digit position turns the balanced digits (each in [-B/2, B/2), carries included) into plain bit fields:
//     digit_j = ((abar + (B/2)(1 + B + .. + B^(l-1))) >> j*beta) mod B - B/2.
// Flipping the top bit of every field then leaves digit_j in two's complement, ready for a signed bit-field extract:
//     fields = (uint32_t)fma(d, scale, offset) ^ sign_bits      (truncation = floor, < 3 * 2^(l*beta)).
// Every term of `offset` is an integer or a half that a double holds exactly, so the order of the additions changes no bit.
// NL: the number of levels where the kernel knows it at compile time (the loop is unrolled); 0: `levels` at run time.
struct BrRounding {
    double scale, offset;
    uint32_t sign_bits;
};
template <int NL = 0>
__device__ __forceinline__ BrRounding br_rounding(uint32_t levels, uint32_t beta) {
    if constexpr (NL != 0) levels = NL;
    const uint32_t bhalf = 1u << (beta - 1);
    BrRounding r{fp_exp2i(-(int)(FQ_BITS - levels * beta)), 0.5 + fp_exp2i((int)(levels * beta)), 0u};
    auto level = [&](uint32_t j) {
        r.offset += (double)(bhalf << (j * beta));
        r.sign_bits |= bhalf << (j * beta);
    };
    if constexpr (NL != 0) {
#pragma unroll
        for (uint32_t j = 0; j < NL; j++) level(j);
    } else {
        for (uint32_t j = 0; j < levels; j++) level(j);
    }
    return r;
}

// Sample extraction of coefficient 0 of a K1-component accumulator (K1 - 1 mask polynomials, then the body), plus the table's
// constant (none where the rotation started from an encrypted sample, a.acc0); the whole epilogue of a kernel.  `comp`
// (wave-uniform): the component this thread holds.
template <int N, int LANES, int K1, int E>
__device__ __forceinline__ void br_extract(const BrArgs &a, const BrJob &job, const double (&acc)[E], uint32_t comp, uint32_t t) {
    if (!job.live) return;
    if (uint64_t *raw = gate_acc(a.gv, job.f, K1 * N)) {   // a rotation of TV_0 that several tables share: the whole accumulator
#pragma unroll
        for (int m = 0; m < E; m++) raw[comp * N + t + (uint32_t)LANES * m] = fp_to_u64(fp_canon(acc[m]));
        return;
    }
    uint64_t *out = gate_out(a.gv, job.f, a.ct_words);
    if (comp < (uint32_t)(K1 - 1)) {
#pragma unroll
        for (int m = 0; m < E; m++) {
            const uint32_t j = t + (uint32_t)LANES * m;
            const uint64_t v = fp_to_u64(fp_canon(acc[m]));
            if (j == 0) out[comp * N] = v;
            else out[comp * N + N - j] = fq_neg(v);
        }
    } else if (t == 0) {
        const uint64_t b = fp_to_u64(fp_canon(acc[0]));
        out[(K1 - 1) * N] = a.post ? fq_add(b, a.post[job.table]) : b;   // (no `post` with acc0: nothing new lives through the steps)
    }
}

// ---------------------------------------------------------------------------------------------
// The one-time transform of a key: `polys` polynomials, coefficient domain -> transform domain, centred, x N^-1, in the register
// order of the transform (key_word) -- the form every kernel multiplies by.  Src yields coefficient j of polynomial p:
// KeyWords for a key of residues (the bootstrapping key, the packing key), KeyBits for a binary secret held as packed bits
// (fbs_keygen.hip).  Workgroups stride over the polynomials.
struct KeyWords {
    const uint64_t *__restrict__ src;   // [polys][N]
    __device__ __forceinline__ double coeff(size_t p, uint32_t n, uint32_t j) const { return fp_from_u64(src[p * n + j]); }
};
struct KeyBits {
    const uint32_t *__restrict__ bits;  // bit p N + j; a secret has at most 4 polynomials: 32-bit indices
    __device__ __forceinline__ double coeff(size_t p, uint32_t n, uint32_t j) const {
        const uint32_t i = (uint32_t)p * n + j;
        return ((bits[i >> 5] >> (i & 31u)) & 1u) ? 1.0 : 0.0;
    }
};
template <int LOGN, int LL, class Src>
__global__ __launch_bounds__(1 << LL) void k_key_transform(Src src, double *__restrict__ dst, const double *__restrict__ tw_fwd,
                                                           double n_inv, size_t polys) {
    using W = typename NttFor<LOGN, LL>::type;
    __shared__ double lds[2 * W::N];
    const uint32_t t = threadIdx.x;
    typename W::Xchg xc{lds, 0};
    for (size_t p = blockIdx.x; p < polys; p += gridDim.x) {   // uniform trip count per workgroup
        double x[W::E];
#pragma unroll
        for (int m = 0; m < W::E; m++) x[m] = src.coeff(p, W::N, W::template index_of<0>(t, m));
        W::forward(x, xc, t, Twiddles(tw_fwd + W::LANE_TABLE_OFFSET, tw_fwd));
#pragma unroll
        for (int m = 0; m < W::E; m++) dst[p * W::N + W::key_word(t, m)] = fp_center(fp_mulmod(x[m], n_inv));
    }
}

// the launch of one descriptor (fbs_select.hpp) in each launch file: false when the descriptor is not of its families
// fbs_blind_rotate_cu.hip: one bootstrap on the eight waves of a CU (k = 1)
bool launch_blind_rotate_cu(const Kernel &k, const BrArgs &a, hipStream_t stream);
// fbs_blind_rotate_k2.hip: GLWE dimension k = 2 at N = 1024, two key bits per step, one gadget level
bool launch_blind_rotate_k2(const Kernel &k, const BrArgs &a, hipStream_t stream);
// fbs_blind_rotate_glwe.hip: every other k >= 2: k + 1 waves per bootstrap, one wave per polynomial
bool launch_blind_rotate_glwe(const Kernel &k, const BrArgs &a, hipStream_t stream);

}  // namespace fbs

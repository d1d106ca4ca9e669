// Test hooks: the FP64 field primitives element by element, and every transform variant a kernel instantiates, run in isolation by one
// workgroup (fbs_debug_field, fbs_debug_transform_list, fbs_debug_transform: include/fbs_exec.h, debug section).  gfx950 only.
//
// A variant is a (transform class, direction, FIRST or BOUNDED[, NP]) that some blind-rotation kernel calls.  The list is made from the
// instantiation lists of fbs_select.hpp -- the ones the kernels are instantiated from -- by the rules the kernel templates apply to their
// arguments (restated in br_first / br_bounded below; tests/test_transform_reference.py holds them against the kernels' source).  A
// kernel added to a list adds its variants here.
//
// What a hook kernel does is what the kernels do around a transform: one exchange buffer per polynomial with the per-lane twiddle
// table of the direction copied into LDS beside it (k_blind_rotate with LL <= FBS_ONE_BUFFER_MAX_LL), the wave-uniform twiddles of the
// inverse requested with inverse_uniform(), the hooks empty; for the wave-private lane transforms, CuTwiddles' init / forward<NP> /
// inverse on the four waves of a polynomial (k_blind_rotate_cu, k_blind_rotate_cu_pairs, k_blind_rotate_cu_k2).  The twiddle tables
// depend on N alone, so a context of the variant's N serves whatever its k.
//
// Conventions (so that no caller needs to know a layout): values are int64 in and out, NOT reduced; the coefficient side is in natural
// order (index_of<0>; a part of a lane transform: element ln + 64 m of part w at word w M + ln + 64 m); the evaluation side is in
// register order, word t E + m = register m of thread t.  What forward leaves in a register is what inverse takes from it.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "fbs_blind_rotate_cu.hpp"

namespace fbs {

// ---- field primitives -----------------------------------------------------------------------------------------------------------
__global__ void k_debug_field(int op, const long long *x, const long long *w, size_t count, long long *out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const double a = (double)x[i], b = w ? (double)w[i] : 0.0;
    long long r = 0;
    switch (op) {
    case 0: r = (long long)fp_mulmod(a, b); break;
    case 1: r = (long long)fp_mulmod_exact(a, b); break;
    case 2: r = (long long)fp_center(a); break;
    case 3: r = (long long)fp_canon(a); break;
    case 4: r = (long long)fp_canon_near(a); break;
    case 5: r = (long long)fp_to_u64(fp_from_u64((uint64_t)x[i])); break;
    }
    out[i] = r;
}

int dev_debug_field(fbs_ctx *ctx, int op, const int64_t *x, const int64_t *w, size_t count, int64_t *out) {
    if (op < 0 || op > 5 || !x || !out || (op <= 1 && !w)) return set_error(ctx, FBS_E_INVALID, "debug_field: bad operation or null array");
    if (count == 0) return FBS_OK;
    if (count > (1u << 26)) return set_error(ctx, FBS_E_INVALID, "debug_field: too many operands");
    const size_t bytes = count * 8;
    long long *d = nullptr;
    FBS_HIP(ctx, hipMalloc(&d, 3 * bytes));
    hipError_t e = hipMemcpy(d, x, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess && w) e = hipMemcpy(d + count, w, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_debug_field, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, ctx->stream, op, d, w ? d + count : nullptr, count,
                           d + 2 * count);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = hipMemcpy(out, d + 2 * count, bytes, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return set_error(ctx, FBS_E_DEVICE, std::string("debug_field: ") + hipGetErrorString(e));
    return FBS_OK;
}

// ---- one polynomial per workgroup on the transform of a shape (PolyNtt / SplitNtt / WavesNtt) -------------------------------------
// LDS as k_blind_rotate lays out a component: [N] exchange buffer, [N] the direction's per-lane twiddle table
template <class W>
__device__ __forceinline__ Twiddles debug_twiddles(double *lds, const double *tw, uint32_t t) {
    static_assert(W::LANES <= (1 << FBS_ONE_BUFFER_MAX_LL), "every shape exchanges through one buffer");
#pragma unroll
    for (int m = 0; m < W::E; m++) lds[W::N + t + (uint32_t)W::LANES * m] = tw[W::LANE_TABLE_OFFSET + t + (uint32_t)W::LANES * m];
    __syncthreads();
    return Twiddles(lds + W::N, tw);
}

template <class W, int FIRST>
__global__ __launch_bounds__(W::LANES) void k_debug_forward(const long long *in, long long *out, const double *tw_fwd, const double *) {
    __shared__ double lds[2 * W::N];
    const uint32_t t = threadIdx.x;
    const Twiddles twf = debug_twiddles<W>(lds, tw_fwd, t);
    typename W::Xchg xc{lds, 0};
    xc.stride = 0;
    const long long *src = in + (size_t)blockIdx.x * W::N;
    long long *dst = out + (size_t)blockIdx.x * W::N;
    double x[W::E];
#pragma unroll
    for (int m = 0; m < W::E; m++) x[m] = (double)src[W::template index_of<0>(t, m)];
    W::template forward<FIRST>(x, xc, t, twf, typename W::NoHook{});
#pragma unroll
    for (int m = 0; m < W::E; m++) dst[t * W::E + m] = (long long)x[m];
}

template <class W, bool BOUNDED>
__global__ __launch_bounds__(W::LANES) void k_debug_inverse(const long long *in, long long *out, const double *, const double *tw_inv) {
    __shared__ double lds[2 * W::N];
    const uint32_t t = threadIdx.x;
    const Twiddles twi = debug_twiddles<W>(lds, tw_inv, t);
    typename W::Xchg xc{lds, 0};
    xc.stride = 0;
    const long long *src = in + (size_t)blockIdx.x * W::N;
    long long *dst = out + (size_t)blockIdx.x * W::N;
    double x[W::E];
#pragma unroll
    for (int m = 0; m < W::E; m++) x[m] = (double)src[t * W::E + m];
    const typename W::InvUniform inv_uni = W::inverse_uniform(t, twi);
    W::template inverse<BOUNDED>(x, xc, t, twi, inv_uni);
#pragma unroll
    for (int m = 0; m < W::E; m++) dst[W::template index_of<0>(t, m)] = (long long)x[m];
}

// SplitNtt::inverse_exit_centred, called as k_blind_rotate calls it where a wave holds a whole polynomial and DIG >= 1
template <class W>
__global__ __launch_bounds__(W::LANES) void k_debug_inverse_exit_centred(const long long *in, long long *out, const double *, const double *tw_inv) {
    __shared__ double lds[2 * W::N];
    const uint32_t t = threadIdx.x;
    const Twiddles twi = debug_twiddles<W>(lds, tw_inv, t);
    typename W::Xchg xc{lds, 0};
    xc.stride = 0;
    const long long *src = in + (size_t)blockIdx.x * W::N;
    long long *dst = out + (size_t)blockIdx.x * W::N;
    double x[W::E];
#pragma unroll
    for (int m = 0; m < W::E; m++) x[m] = (double)src[t * W::E + m];
    const typename W::InvUniform inv_uni = W::inverse_uniform(t, twi);
    W::inverse_exit_centred(x, xc, t, twi, inv_uni);
#pragma unroll
    for (int m = 0; m < W::E; m++) dst[W::template index_of<0>(t, m)] = (long long)x[m];
}

// ---- the wave-private lane transforms: the four parts of a polynomial on four waves, NP polynomials side by side -------------------
template <int LOGN, int NP>
__global__ __launch_bounds__(256) void k_debug_lane_forward(const long long *in, long long *out, const double *tw_fwd, const double *tw_inv) {
    using W = WavesNtt<LOGN, 2>;
    using Part = typename W::Half;
    constexpr int N = W::N, E = W::E, M = W::M;
    __shared__ double lds[NP * N + CuTwiddles<Part, false>::LDS_WORDS];
    const uint32_t t = threadIdx.x, w = W::wave_of(t), ln = t & 63u;
    CuTwiddles<Part, false> tw;
    tw.init((uniform_doubles)(uintptr_t)tw_fwd, (uniform_doubles)(uintptr_t)tw_inv, tw_fwd + W::LANE_TABLE_OFFSET, tw_inv + W::LANE_TABLE_OFFSET, w,
            ln, lds + NP * N);
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * NP * N;
    double x[NP][E];
    double *bufs[NP];
#pragma unroll
    for (int p = 0; p < NP; p++) {
        bufs[p] = lds + p * N + w * M;
#pragma unroll
        for (int m = 0; m < E; m++) x[p][m] = (double)in[base + (size_t)p * N + w * M + ln + 64u * m];
    }
    tw.template forward<NP>(x, bufs, ln);
#pragma unroll
    for (int p = 0; p < NP; p++)
#pragma unroll
        for (int m = 0; m < E; m++) out[base + (size_t)p * N + t * E + m] = (long long)x[p][m];
}

template <int LOGN>
__global__ __launch_bounds__(256) void k_debug_lane_inverse(const long long *in, long long *out, const double *tw_fwd, const double *tw_inv) {
    using W = WavesNtt<LOGN, 2>;
    using Part = typename W::Half;
    constexpr int N = W::N, E = W::E, M = W::M;
    __shared__ double lds[N + CuTwiddles<Part, false>::LDS_WORDS];
    const uint32_t t = threadIdx.x, w = W::wave_of(t), ln = t & 63u;
    CuTwiddles<Part, false> tw;
    tw.init((uniform_doubles)(uintptr_t)tw_fwd, (uniform_doubles)(uintptr_t)tw_inv, tw_fwd + W::LANE_TABLE_OFFSET, tw_inv + W::LANE_TABLE_OFFSET, w,
            ln, lds + N);
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * N;
    double x[E];
#pragma unroll
    for (int m = 0; m < E; m++) x[m] = (double)in[base + t * E + m];
    tw.inverse(x, lds + w * M, ln, typename Part::NoHook{});
#pragma unroll
    for (int m = 0; m < E; m++) out[base + w * M + ln + 64u * m] = (long long)x[m];
}

// ---- the variants ---------------------------------------------------------------------------------------------------------------
// what the kernel templates derive from their arguments (k_blind_rotate, k_blind_rotate_pairs: fbs_blind_rotate.hip)
template <class W>
constexpr int br_first(int dig) {
    return (dig == 3 || dig == 7) ? (has_fused_opening<W>::value ? 3 : 2) : (dig == 2 || dig == 6) ? 1 : 0;
}
constexpr bool br_bounded(int dig) { return dig >= 1; }
constexpr int pairs_first(int dig) { return dig == 3 ? 2 : 0; }

template <class W>
struct NttClass;
template <int LOGN, int LL>
struct NttClass<PolyNtt<LOGN, LL>> {
    static constexpr const char *name = "PolyNtt";
    static constexpr int logn = LOGN;
};
template <int LOGN, int LL>
struct NttClass<SplitNtt<LOGN, LL>> {
    static constexpr const char *name = "SplitNtt";
    static constexpr int logn = LOGN;
};
template <int LOGN, int LOGW>
struct NttClass<WavesNtt<LOGN, LOGW>> {
    static constexpr const char *name = "WavesNtt";
    static constexpr int logn = LOGN;
};
template <class Part>
constexpr const char *lane_class() {
    return std::is_same<Part, LaneNtt256>::value ? "LaneNtt256" : "LaneNtt512";
}

typedef void (*DebugKernel)(const long long *, long long *, const double *, const double *);
struct Variant {
    std::string line;
    int logn, lanes, np;   // np: polynomials a workgroup takes
    DebugKernel kernel;
    bool listed = true;    // named by fbs_debug_transform_list (false: fbs_debug_transform runs it all the same)
};

static void add(std::vector<Variant> &v, const char *cls, int logn, int lanes, const char *dir, const char *what, int value, int np,
                DebugKernel kernel) {
    char text[128];
    int len = snprintf(text, sizeof text, "class=%s logn=%d lanes=%d dir=%s %s=%d", cls, logn, lanes, dir, what, value);
    if (np) snprintf(text + len, sizeof text - len, " np=%d", np);
    for (const Variant &have : v)
        if (have.line == text) return;
    v.push_back({text, logn, lanes, np ? np : 1, kernel});
}
template <class W, int FIRST>
static void add_forward(std::vector<Variant> &v) {
    add(v, NttClass<W>::name, NttClass<W>::logn, W::LANES, "forward", "first", FIRST, 0, k_debug_forward<W, FIRST>);
}
template <class W, bool BOUNDED>
static void add_inverse(std::vector<Variant> &v) {
    add(v, NttClass<W>::name, NttClass<W>::logn, W::LANES, "inverse", "bounded", BOUNDED, 0, k_debug_inverse<W, BOUNDED>);
}
// the whole-CU kernels run the cross stages themselves and call the lane transform with FIRST = 0 whatever their digits
template <int LOGN, int NP>
static void add_lane(std::vector<Variant> &v) {
    using Part = typename WavesNtt<LOGN, 2>::Half;
    add(v, lane_class<Part>(), LOGN, 256, "forward", "first", 0, NP, k_debug_lane_forward<LOGN, NP>);
    add(v, lane_class<Part>(), LOGN, 256, "inverse", "bounded", 0, 0, k_debug_lane_inverse<LOGN>);
}

static const std::vector<Variant> &variants() {
    static const std::vector<Variant> all = [] {
        std::vector<Variant> v;
#define X(L, LL, DIG, FPW, TURNS)                                                       \
    add_forward<typename NttFor<L, LL>::type, br_first<typename NttFor<L, LL>::type>(DIG)>(v); \
    add_inverse<typename NttFor<L, LL>::type, br_bounded(DIG)>(v);
        FBS_BR_KERNELS(X)
#undef X
#define X(L, DIG)                                                                       \
    add_forward<typename NttFor<L, lanes_log2_for(L)>::type, pairs_first(DIG)>(v);      \
    add_inverse<typename NttFor<L, lanes_log2_for(L)>::type, true>(v);
        FBS_PAIRS_KERNELS(X)
#undef X
#define X(L, FPW)                        \
    add_forward<SplitNtt<L, 6>, 0>(v);   \
    add_inverse<SplitNtt<L, 6>, true>(v);
        FBS_PAIRS_K2_KERNELS(X)
#undef X
#define X(L, K1)                                            \
    add_forward<typename NttFor<L, 6>::type, 0>(v);         \
    add_inverse<typename NttFor<L, 6>::type, false>(v);
        FBS_GLWE_SHAPES(X)
#undef X
#define X(L, NL, FIRST, LEAN) add_lane<L, NL>(v);
        FBS_CU_KERNELS(X)
#undef X
#define X(L, NL) add_lane<L, NL>(v);
        FBS_CU_PAIRS_KERNELS(X)
#undef X
        add_lane<10, 1>(v);   // k_blind_rotate_cu_k2 (Family::CU_K2: not a template)
        // Accepted by fbs_debug_transform, NOT named by fbs_debug_transform_list: the list is one forward and one inverse line per
        // kernel by (class, N, lanes, FIRST or BOUNDED) -- what tests/test_transform_reference.py derives from a kernel's name --
        // and k_blind_rotate<10,6,DIG >= 1,.> keeps its "bounded=1" line there, which SplitNtt::inverse<true> still answers (the
        // pairs kernels call it).  The inverse those kernels take instead is this line (tests/test_exit_centred_inverse.py).
        v.push_back({"class=SplitNtt logn=10 lanes=64 dir=inverse bounded=1 centre=exit", 10, 64, 1, k_debug_inverse_exit_centred<SplitNtt<10, 6>>,
                     false});
        return v;
    }();
    return all;
}

const char *debug_transform_list() {
    static const std::string text = [] {
        std::string t;
        for (const Variant &v : variants())
            if (v.listed) t += v.line + "\n";
        return t;
    }();
    return text.c_str();
}

int dev_debug_transform(fbs_ctx *ctx, const char *variant, const int64_t *in, int64_t *out, size_t polys) {
    if (!variant || !in || !out) return set_error(ctx, FBS_E_INVALID, "debug_transform: null argument");
    const Variant *v = nullptr;
    for (const Variant &have : variants())
        if (have.line == variant) v = &have;
    if (!v) return set_error(ctx, FBS_E_INVALID, std::string("debug_transform: no such variant: ") + variant);
    if ((int)ctx->p.log_n_poly != v->logn) return set_error(ctx, FBS_E_INVALID, "debug_transform: the context is of another N");
    if (polys == 0 || polys % (size_t)v->np || polys > 4096) return set_error(ctx, FBS_E_INVALID, "debug_transform: polys must be a multiple of np, at most 4096");
    const size_t words = polys * ctx->N;
    long long *d = nullptr;
    FBS_HIP(ctx, hipMalloc(&d, 2 * words * 8));
    hipError_t e = hipMemcpy(d, in, words * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(v->kernel, dim3((unsigned)(polys / (size_t)v->np)), dim3((unsigned)v->lanes), 0, ctx->stream, d, d + words,
                           reinterpret_cast<const double *>(ctx->d_tw_fwd), reinterpret_cast<const double *>(ctx->d_tw_inv));
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = hipMemcpy(out, d + words, words * 8, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return set_error(ctx, FBS_E_DEVICE, std::string("debug_transform: ") + hipGetErrorString(e));
    return FBS_OK;
}

}  // namespace fbs

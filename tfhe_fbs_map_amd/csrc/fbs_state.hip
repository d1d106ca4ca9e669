// The device-side inputs and outputs of a chunk, gfx950: ciphertexts between the wire slots [n_slots][Tc][D + 1] of a chunk and the
// rows of state blocks [rows][T][D + 1] (fbs_state, fbs_eval_resident, fbs_eval_resident_mapped), and the plaintext inputs of a chunk
// (FBS_SRC_PLAIN) written into the same slots.  One list of links (WireLink, fbs_internal.hpp) says what goes where:
//
//   k_wire_load    wire slot of link e, sample q  <-  row of link e, sample index[s0 + q] (no index: sample s0 + q); or, where the
//                  link has no row or the entry is FBS_SAMPLE_NONE, the trivial ciphertext (D zero words, then the body) of the
//                  link's message for sample q, m Delta mod q, or of its one body.  Every input of a chunk that is made on the
//                  device: state rows read as they are or ACROSS samples, plaintext messages.
//   k_wire_store   row of link e, sample s0 + q   <-  wire slot of link e, sample q    (the outputs into a state; a constant output
//                  is written as the trivial ciphertext fbs_eval returns for it)
//
// One launch moves every link of the chunk: the (link, sample) grid is dealt to waves, one ciphertext per wave at a time, and what
// a wave does with it is one wave-uniform decision (one index word per ciphertext).  A ciphertext is D + 1 words, an odd number, so
// one at an odd index starts 8 bytes off a 16-byte line.  Where source and destination agree in that, the wave moves 16 bytes a
// lane each way, with the one word before or after the pairs on its own (as k_expand_seeded stores its blocks); where they differ
// -- through an index both cases occur within one row -- the stores stay 16 bytes wide and aligned and each takes two 8-byte loads,
// consecutive lanes on consecutive words either way.  Plain vector loads and stores only.  These kernels are copies: they are not
// in fbs_kernel_catalog and the profile does not count them.
//
//   k_state_sum_groups   row r, sample j of dst  <-  the word-wise sum mod q of samples [j group, (j + 1) group) of row r of src
//                        (fbs_state_sum_groups; a streaming reduction: every source word is read once; no LDS, no atomics).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fbs_rows.hpp"

namespace fbs {

constexpr uint32_t ST_WAVES = 4;              // waves (ciphertexts in flight) per workgroup
constexpr uint32_t ST_MAX_BLOCKS = 1u << 16;  // grid cap; the waves stride over the rest

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

// A trivial ciphertext is a pure streaming write, its body -- the only non-zero word -- one value per ciphertext.  m < 2p (checked
// by the host) and Delta <= q / 2p + 1, so m Delta < q + 2p fits 64 bits and one 64-bit remainder is the residue fbs_eval's
// trivial_body computes.
__global__ __launch_bounds__(64 * ST_WAVES) void k_wire_load(WireCopy a) {
    const uint32_t lane = threadIdx.x & 63u, words = a.D + 1;
    const size_t total = a.n_links * a.tc;
    for (size_t c = (size_t)blockIdx.x * ST_WAVES + threadIdx.x / 64; c < total; c += (size_t)gridDim.x * ST_WAVES) {   // wave-uniform
        const size_t e = c / a.tc, q = c - e * a.tc;
        const WireLink ln = a.links[e];
        size_t from = a.s0 + q;
        bool none = !ln.row;
        if (ln.row && ln.index) {   // (one word for the wave; below the row's samples, or FBS_SAMPLE_NONE: the host checked)
            const uint32_t j = ln.index[from];
            from = j, none = j == FBS_SAMPLE_NONE;
        }
        uint64_t *dst = a.wires + ((size_t)ln.slot * a.Tc + q) * words;
        if (none) wave_fill_trivial(dst, ln.msgs ? (uint64_t)ln.msgs[q] * a.delta % FQ : ln.body, words, lane);
        else wave_copy_ct(dst, ln.row + from * words, words, lane);
    }
}

__global__ __launch_bounds__(64 * ST_WAVES) void k_wire_store(WireCopy a) {
    const uint32_t lane = threadIdx.x & 63u, words = a.D + 1;
    const size_t total = a.n_links * a.tc;
    for (size_t c = (size_t)blockIdx.x * ST_WAVES + threadIdx.x / 64; c < total; c += (size_t)gridDim.x * ST_WAVES) {   // wave-uniform
        const size_t e = c / a.tc, q = c - e * a.tc;
        const WireLink ln = a.links[e];
        uint64_t *dst = ln.row + (a.s0 + q) * words;
        if (ln.slot == WIRE_NO_SLOT) wave_fill_trivial(dst, ln.body, words, lane);
        else wave_copy_ct(dst, a.wires + ((size_t)ln.slot * a.Tc + q) * words, words, lane);
    }
}

// One wave takes one (row, output sample, slab) item: a slab is SG_SLAB_PAIRS 16-byte pairs of the output ciphertext, one pair a
// lane -- 1 KiB a wave instruction, the widest global access there is -- so a ciphertext of D + 1 words gives ceil(D / 256) items and
// a launch with few output ciphertexts still spreads over the chip.  The pairs are aligned to the DESTINATION (head word first where
// it starts 8 bytes off a line, as wave_copy_ct); a source sample whose start agrees with that is read 16 bytes a lane, one that
// does not (every other sample: D + 1 is odd) 8 bytes a lane twice, consecutive lanes on consecutive words either way.  The word
// the pairs leave (the first or the last) rides on lane 63 of slab 0.  Each lane walks its group's samples with 64-bit sums:
// group <= 65536 residues below q < 2^46 stay below 2^62, so one remainder at the end gives the canonical sum.
constexpr uint32_t SG_SLAB_PAIRS = 64;

__global__ __launch_bounds__(64 * ST_WAVES) void k_state_sum_groups(SumGroups a) {
    const uint32_t lane = threadIdx.x & 63u, words = a.D + 1;
    const uint32_t pairs = (words - 1) / 2;   // (words odd: the same with and without a head word)
    const uint32_t slabs = std::max(1u, (pairs + SG_SLAB_PAIRS - 1) / SG_SLAB_PAIRS);
    const size_t total = a.rows * a.T_dst * slabs;
    for (size_t c = (size_t)blockIdx.x * ST_WAVES + threadIdx.x / 64; c < total; c += (size_t)gridDim.x * ST_WAVES) {   // wave-uniform
        const size_t rj = c / slabs, r = rj / a.T_dst, j = rj - r * a.T_dst;
        const uint32_t slab = (uint32_t)(c - rj * slabs);
        uint64_t *dst = a.dst + (r * a.T_dst + j) * words;
        const uint32_t head = (uint32_t)(((uintptr_t)dst >> 3) & 1u);
        const uint32_t pr = slab * SG_SLAB_PAIRS + lane, w = head + 2 * pr;   // this lane's pair: words w, w + 1
        const bool paired = pr < pairs, single = slab == 0 && lane == 63;
        const uint32_t ws = head ? 0 : words - 1;                             // the word the pairs leave
        const size_t s_begin = j * a.group, s_end = std::min(s_begin + a.group, a.T_src);
        const uint64_t *ct = a.src + (r * a.T_src + s_begin) * words;
        uint64_t acc0 = 0, acc1 = 0, accs = 0;
#pragma unroll 4
        for (size_t s = s_begin; s < s_end; s++, ct += words) {
            if (paired) {
                const uint64_t *p = ct + w;
                if (((uintptr_t)p & 15u) == 0) {   // wave-uniform
                    const u64x2 v = *reinterpret_cast<const u64x2 *>(p);
                    acc0 += v.x, acc1 += v.y;
                } else {
                    acc0 += p[0], acc1 += p[1];
                }
            }
            if (single) accs += ct[ws];
        }
        if (paired) *reinterpret_cast<u64x2 *>(dst + w) = u64x2{acc0 % FQ, acc1 % FQ};
        if (single) dst[ws] = accs % FQ;
    }
}

static dim3 st_grid(size_t total) { return dim3((unsigned)std::min<size_t>((total + ST_WAVES - 1) / ST_WAVES, ST_MAX_BLOCKS)); }

static int launch_links(const fbs_ctx *ctx, void (*kernel)(WireCopy), const WireCopy &a, hipStream_t stream) {
    if (a.n_links * a.tc == 0) return FBS_OK;
    hipLaunchKernelGGL(kernel, st_grid(a.n_links * a.tc), dim3(64 * ST_WAVES), 0, stream, a);
    FBS_HIP(ctx, hipGetLastError());
    return FBS_OK;
}

int dev_wire_load(const fbs_ctx *ctx, const WireCopy &a, hipStream_t stream) { return launch_links(ctx, k_wire_load, a, stream); }

int dev_wire_store(const fbs_ctx *ctx, const WireCopy &a, hipStream_t stream) { return launch_links(ctx, k_wire_store, a, stream); }

int dev_state_sum_groups(const fbs_ctx *ctx, const SumGroups &a, hipStream_t stream) {
    const size_t pairs = a.D / 2, slabs = std::max<size_t>(1, (pairs + SG_SLAB_PAIRS - 1) / SG_SLAB_PAIRS);
    if (a.rows * a.T_dst == 0) return FBS_OK;
    hipLaunchKernelGGL(k_state_sum_groups, st_grid(a.rows * a.T_dst * slabs), dim3(64 * ST_WAVES), 0, stream, a);
    FBS_HIP(ctx, hipGetLastError());
    return FBS_OK;
}

}  // namespace fbs

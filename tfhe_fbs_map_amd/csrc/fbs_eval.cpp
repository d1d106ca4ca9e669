// The whole-program evaluations of libfbsexec.so (declared in include/fbs_exec.h): the level-scheduled executor that stands behind
// `LutExecEnv.eval` (reference fbs_mapper/fbs_exec_env.py:208-229).  One chunk loop (eval_chunks) serves every entry.  fbs_eval_dev
// and fbs_eval_messages bring load and store stages of their own; every other entry -- fbs_eval, fbs_eval_seeded,
// fbs_eval_seeded_compact, fbs_eval_sources, fbs_eval_resident -- is eval_sources.  The level calls, the scratch helpers and the
// rest of the ABI are fbs_capi.cpp's.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <functional>

#include "fbs_api_checks.hpp"
#include "fbs_compact.hpp"
#include "fbs_internal.hpp"

using namespace fbs;

static int run_levels(fbs_ctx *ctx, const fbs_prog *prog, uint64_t *d_wires, size_t T, size_t s_count, hipStream_t s) {
    int rc;
    for (uint32_t L = 0; L <= prog->depth; L++) {
        if ((rc = fbs_level_lincomb_dev(ctx, prog, L, d_wires, T, 0, s_count, s)) != FBS_OK) return rc;
        if (L == prog->depth) break;
        const size_t total = (size_t)prog->boot[L].n_gates * s_count;
        if ((rc = fbs_level_bootstrap_dev(ctx, prog, L, d_wires, T, 0, s_count, 0, total, nullptr, s)) != FBS_OK) return rc;
    }
    return FBS_OK;
}

// Samples are independent through the whole program: evaluate in chunks whose wire slots fit in HBM.  The wire buffer
// belongs to the context and is shared by all of its programs (it only ever grows).
// `extra_per_sample`: bytes per sample of a further buffer the caller sizes by the chunk (the packed staging of compact outputs)
static int reserve_wires(fbs_ctx *ctx, const fbs_prog *prog, size_t T, size_t *chunk, size_t extra_per_sample = 0) {
    const size_t ctw = ctx->D + 1;
    const size_t per_sample = (size_t)prog->n_slots * ctw * 8 + (size_t)std::max(1u, prog->max_sources) * (ctx->p.n + 1) * 4 +
                              (size_t)prog->max_shared * (ctx->p.k + 1) * ctx->N * 8 + extra_per_sample;
    size_t free_b = 0, total_b = 0;
    FBS_HIP(ctx, hipMemGetInfo(&free_b, &total_b));
    size_t have = free_b + ctx->wires_capacity * 8 + ctx->ms_capacity * (ctx->p.n + 1) * 4 + ctx->acc_capacity * (size_t)(ctx->p.k + 1) * ctx->N * 8;
    if (extra_per_sample) have += ctx->compact_capacity * 8;   // (the compact path reuses its packed staging; no other call does)
    // test hook: FBS_WIRE_BUDGET_MB caps what the wire slots may take, so that the chunked path runs at small sizes
    if (const char *cap = getenv("FBS_WIRE_BUDGET_MB")) have = std::min<size_t>(have, (size_t)std::max(1, atoi(cap)) << 20);
    const size_t Tc = std::min<size_t>(T, std::max<size_t>(1, (size_t)(0.6 * (double)have) / per_sample));
    const size_t words = Tc * (size_t)prog->n_slots * ctw;
    int rc = ensure_wires(ctx, words);
    if (rc != FBS_OK) return rc;
    rc = ensure_ms(ctx, (size_t)std::max(1u, prog->max_sources) * Tc);
    if (rc != FBS_OK) return rc;
    if (prog->max_shared && (rc = ensure_acc(ctx, (size_t)prog->max_shared * Tc)) != FBS_OK) return rc;
    *chunk = Tc;
    return FBS_OK;
}

static uint64_t trivial_body(const fbs_ctx *ctx, int64_t out_slot) { return fq_mul(fq_from_i64(-1 - out_slot), 2 * ctx->delta_half); }
// the body of the trivial ciphertext of a message m in [0, 2p): m Delta mod q, as k_wire_load works it out for a message per sample
static uint64_t message_body(const fbs_ctx *ctx, int64_t m) { return (uint64_t)m * (2 * ctx->delta_half) % FQ; }

// ---- the program evaluations: one chunk loop, each entry its checks, its scratch and its two stages -------------------------
// what every evaluation checks first: the keys, the program's owner, the buffers of a call with samples
static int check_eval(fbs_ctx *ctx, const fbs_prog *prog, const void *in, size_t T, const void *out) {
    if (int rc = check_prog(ctx, prog)) return rc;
    if (T && ((prog->n_inputs && !in) || (prog->n_outputs && !out))) return set_error(ctx, FBS_E_INVALID, "null argument");
    return FBS_OK;
}

// samples [s0, s0 + tc) of the chunk: put the inputs into their wire slots, or take the outputs out of theirs
using ChunkStage = std::function<int(size_t s0, size_t tc)>;

// Chunks of Tc samples (reserve_wires) on stream `s`: load, run_levels, store.  `sync`: the host-facing entries wait for each
// chunk (pageable memory), then run `post` on it when given; fbs_eval_dev only launches.  A failure inside the loop puts the
// scratch back (scratch_fail).
static int eval_chunks(fbs_ctx *ctx, const fbs_prog *prog, size_t T, size_t Tc, hipStream_t s, bool sync, const ChunkStage &load,
                       const ChunkStage &store, const ChunkStage &post = nullptr) {
    int rc;
    if ((rc = scratch_wait(ctx, s)) != FBS_OK) return rc;
    for (size_t s0 = 0; s0 < T; s0 += Tc) {
        const size_t tc = std::min(Tc, T - s0);
        if ((rc = load(s0, tc)) || (rc = run_levels(ctx, prog, ctx->d_wires, Tc, tc, s)) || (rc = store(s0, tc))) return scratch_fail(ctx, s, rc);
        if (sync && ((rc = sync_stream(ctx, s)) || (post && (rc = post(s0, tc))))) return scratch_fail(ctx, s, rc);
    }
    return scratch_done(ctx, s);
}

// the output slots -> host ciphertexts [n_outputs][T][D + 1]; a constant output as its trivial ciphertext
static int store_host_cts(fbs_ctx *ctx, const fbs_prog *prog, uint64_t *out, size_t T, size_t Tc, size_t s0, size_t tc, hipStream_t s) {
    const size_t ctw = ctx->D + 1;
    for (uint32_t o = 0; o < prog->n_outputs; o++) {
        uint64_t *dst = out + ((size_t)o * T + s0) * ctw;
        const int64_t w = prog->out_slot[o];
        if (w >= 0) {
            FBS_HIP(ctx, hipMemcpyAsync(dst, ctx->d_wires + (size_t)w * Tc * ctw, tc * ctw * 8, hipMemcpyDeviceToHost, s));
        } else {
            const uint64_t body = trivial_body(ctx, w);
            for (size_t q = 0; q < tc; q++) {
                std::memset(dst + q * ctw, 0, ctx->D * 8);
                dst[q * ctw + ctx->D] = body;
            }
        }
    }
    return FBS_OK;
}

// The compact store stage (out_bits != 0): the output slots of a chunk are key-switched and packed on the device in groups of
// outputs whose rows fit the modulus-switch scratch reserve_wires sized (max_sources x Tc rows), and only the packed words are
// copied back; a constant output is the compaction of the trivial ciphertext store_host_cts writes for it.
// The caller counts the packed staging (cap_rows x W words) in the chunk's budget and grows d_compact to it.
struct CompactStore {
    uint32_t bits = 0;
    size_t W = 0, cap_rows = 0;
    std::vector<uint64_t> constant;   // [n_outputs][W]
};
static CompactStore compact_store_for(const fbs_ctx *ctx, const fbs_prog *prog, uint32_t bits, size_t Tc) {
    CompactStore cs;
    cs.bits = bits;
    cs.W = compact_words(ctx->p.n, bits);
    cs.cap_rows = (size_t)std::max(1u, prog->max_sources) * Tc;   // (ensure_ms has made d_ms at least this long)
    cs.constant.assign((size_t)prog->n_outputs * cs.W, 0);
    for (size_t o = 0; o < prog->n_outputs; o++)
        if (prog->out_slot[o] < 0) host_compact_trivial(ctx, trivial_body(ctx, prog->out_slot[o]), bits, cs.constant.data() + o * cs.W);
    return cs;
}
static int store_compact(fbs_ctx *ctx, const fbs_prog *prog, const CompactStore &cs, uint64_t *out_words, size_t T, size_t Tc,
                         size_t s0, size_t tc, hipStream_t s) {
    const size_t W = cs.W, n_live = prog->live_out.size(), group = std::max<size_t>(1, cs.cap_rows / tc);
    for (size_t g0 = 0; g0 < n_live; g0 += group) {
        const size_t ng = std::min(group, n_live - g0), rows = ng * tc;
        const GateView gv = slots_view(ctx->d_wires, nullptr, prog->d_live_slot + g0, ng, Tc, tc);
        if (int rc = dev_keyswitch(ctx, gv, ctx->d_ms, cs.bits, s)) return rc;
        if (int rc = dev_compact_pack(ctx, ctx->d_ms, rows, cs.bits, ctx->d_compact, s)) return rc;
        for (size_t i = 0; i < ng; i++)
            FBS_HIP(ctx, hipMemcpyAsync(out_words + ((size_t)prog->live_out[g0 + i] * T + s0) * W, ctx->d_compact + i * tc * W, tc * W * 8,
                                        hipMemcpyDeviceToHost, s));
    }
    for (size_t o = 0; o < prog->n_outputs; o++)
        if (prog->out_slot[o] < 0)
            for (size_t q = 0; q < tc; q++) std::memcpy(out_words + (o * T + s0 + q) * W, cs.constant.data() + o * W, W * 8);
    return FBS_OK;
}

// ---- eval_sources: programs over mixed input sources, the evaluation behind every host-buffer entry ---------------------------
// One more pair of stages on eval_chunks.  Load: the steps below, in their order; compact inputs and inputs marked `refresh` are
// refreshed in groups whose rows fit the scratch reserve_wires sized (max_sources x Tc rows).  Store: full ciphertexts
// (store_host_cts), compact ones (store_compact), or -- fbs_eval_resident's out_state -- one store launch per chunk (k_wire_store) into a state.
// With out_state and no full or compact host input (plaintext messages are none) nothing has to come back: the chunks are queued
// without waiting, and the call returns once the arrays it was given have been read (`inputs_event`, after the last chunk's load).
//
// What a call does, worked out from its arguments alone (plan_sources), then what it reserved (reserve_sources):
struct SourcePlan {
    const fbs_prog *prog = nullptr;   // the call's arguments
    const fbs_input_src *src = nullptr;
    const fbs_resident_src *res = nullptr;
    const fbs_sample_map *maps = nullptr;
    size_t T = 0;
    uint32_t out_bits = 0;
    size_t W_in = 0, W_out = 0;                             // words of the widest compact input, of a compact output (0: none)
    std::vector<uint32_t> compact_in, full_refresh;         // input indices by kind
    bool any_seeded = false, host_cts = false;              // host_cts: some input is ciphertexts in host memory
    std::vector<WireLink> links;                            // the input links [n_in_links], in input order, then the output links
    size_t n_in_links = 0;
    struct At {
        uint32_t input, link;
    };
    // the links reserve_sources patches a device address into, with their inputs: those with a sample map (map j of the call lies
    // at d_idx + refresh slots + j T), those of plaintext inputs that bring a message per sample (at d_io_msgs + input Tc)
    std::vector<At> mapped, msgs;
    std::vector<uint32_t> refresh_slot;                     // the slots to refresh, compact inputs first
    bool wait = true;                                       // results or pageable ciphertexts cross the bus: chunk by chunk
    // reserve_sources: the chunk, the rows of the modulus-switch scratch a group of refreshes may fill, the identity table
    size_t Tc = 0, cap_rows = 0;
    const fbs_tvset *tv = nullptr;
    CompactStore cs;

    bool resident(size_t i) const { return res && res[i].state; }
    bool has_map(size_t i) const { return maps && maps[i].index; }
    bool from(size_t i, uint32_t kind) const { return !resident(i) && src[i].kind == kind; }
    bool per_sample(size_t i) const { return from(i, FBS_SRC_PLAIN) && !src[i].bits; }
};
struct Chunk {   // samples [s0, s0 + tc) in wire slots of Tc samples, queued on s
    size_t Tc, s0, tc;
    hipStream_t s;
};

// every argument is checked before anything is reserved, copied or launched
static int plan_sources(const fbs_ctx *ctx, const fbs_prog *prog, const fbs_input_src *src, const fbs_resident_src *res,
                        const fbs_sample_map *maps, size_t T, uint32_t out_bits, const uint64_t *out, const fbs_state *out_state, SourcePlan &p) {
    p.prog = prog, p.src = src, p.res = res, p.maps = maps, p.T = T, p.out_bits = out_bits;
    int rc;
    if (out_bits && (rc = check_bits(ctx, out_bits)) != FBS_OK) return rc;
    if (out_state) {
        if (!state_of(ctx, out_state)) return set_error(ctx, FBS_E_INVALID, "the output state is not a live state of this context");
        if (out_bits) return set_error(ctx, FBS_E_INVALID, "outputs into a state are full ciphertexts: out_bits must be 0");
        if (out_state->rows != prog->n_outputs)
            return set_error(ctx, FBS_E_INVALID, "the output state has " + std::to_string(out_state->rows) + " rows for " +
                                                     std::to_string(prog->n_outputs) + " outputs");
        if (out_state->T != T) return set_error(ctx, FBS_E_INVALID, "the output state holds " + std::to_string(out_state->T) + " samples a row, the call has " + std::to_string(T));
    }
    for (size_t i = 0; (res || maps) && i < prog->n_inputs; i++) {
        const fbs_state *st = res ? res[i].state : nullptr;
        if (!st && !p.has_map(i)) continue;
        const std::string who = "input " + std::to_string(i) + ": ";
        if (!st) return set_error(ctx, FBS_E_INVALID, who + "a sample map on an input that is not a state row");
        if (!state_of(ctx, st)) return set_error(ctx, FBS_E_INVALID, who + "not a live state of this context");
        if (st == out_state) return set_error(ctx, FBS_E_INVALID, who + "the output state is also an input state (no in-place hops)");
        if (res[i].row >= st->rows) return set_error(ctx, FBS_E_INVALID, who + "row " + std::to_string(res[i].row) + " of a state of " + std::to_string(st->rows) + " rows");
        if (!p.has_map(i)) {
            if (st->T != T) return set_error(ctx, FBS_E_INVALID, who + "its state holds " + std::to_string(st->T) + " samples a row, the call has " + std::to_string(T));
            continue;
        }
        // a mapped input: sample s is sample index[s] of the row, or the trivial ciphertext of `fill`
        if (maps[i].fill < 0 || maps[i].fill >= 2 * (int64_t)ctx->p.p_msg)
            return set_error(ctx, FBS_E_INVALID, who + "fill " + std::to_string(maps[i].fill) + " outside [0, 2p)");
        for (size_t s = 0; s < T; s++)
            if (maps[i].index[s] != FBS_SAMPLE_NONE && maps[i].index[s] >= st->T)
                return set_error(ctx, FBS_E_INVALID, who + "sample " + std::to_string(s) + " reads sample " + std::to_string(maps[i].index[s]) +
                                                         " of a state of " + std::to_string(st->T) + " a row");
    }
    if (T == 0) return FBS_OK;
    const size_t n_in = prog->n_inputs, n_out = prog->n_outputs, ctw = ctx->D + 1;
    bool from_src = false;
    for (size_t i = 0; i < n_in; i++) from_src |= !p.resident(i);
    if ((from_src && !src) || (n_out && !out && !out_state)) return set_error(ctx, FBS_E_INVALID, "null argument");
    p.W_out = out_bits ? compact_words(ctx->p.n, out_bits) : 0;
    for (size_t i = 0; i < n_in; i++) {
        if (p.resident(i)) {
            // (a mapped link's index is filled in by reserve_sources; its fill body is what FBS_SRC_PLAIN writes for that message)
            if (p.has_map(i)) p.mapped.push_back({(uint32_t)i, (uint32_t)p.links.size()});
            p.links.push_back(WireLink{res[i].state->d + (size_t)res[i].row * res[i].state->T * ctw, nullptr, nullptr,
                                       p.has_map(i) ? message_body(ctx, maps[i].fill) : 0, prog->in_slot[i]});
            if (res[i].refresh) p.full_refresh.push_back((uint32_t)i);
            continue;
        }
        const fbs_input_src &x = src[i];
        const std::string who = "input " + std::to_string(i) + ": ";
        if (x.kind > FBS_SRC_PLAIN) return set_error(ctx, FBS_E_INVALID, who + "unknown source kind " + std::to_string(x.kind));
        if (!x.data) return set_error(ctx, FBS_E_INVALID, who + "null data");
        if (x.kind == FBS_SRC_PLAIN) {   // cleartext messages: [T], or one for every sample (bits = 1)
            if (x.refresh) return set_error(ctx, FBS_E_INVALID, who + "a plaintext input is not refreshed");
            if (x.bits > 1) return set_error(ctx, FBS_E_INVALID, who + "bits of a plaintext input is 0 ([T] messages) or 1 (one message for all)");
            if (T > SIZE_MAX / 8) return set_error(ctx, FBS_E_INVALID, who + "T * words overflow");
            const int64_t *m = reinterpret_cast<const int64_t *>(x.data);
            for (size_t q = 0, count = x.bits ? 1 : T; q < count; q++)
                if (m[q] < 0 || m[q] >= 2 * (int64_t)ctx->p.p_msg)
                    return set_error(ctx, FBS_E_INVALID, who + "message " + std::to_string(m[q]) + " outside [0, 2p)");
            // (a per-sample input's messages lie where its bodies would: reserve_sources fills in the device address)
            if (!x.bits) p.msgs.push_back({(uint32_t)i, (uint32_t)p.links.size()});
            p.links.push_back(WireLink{nullptr, nullptr, nullptr, x.bits ? message_body(ctx, m[0]) : 0, prog->in_slot[i]});
            continue;
        }
        size_t words = x.kind == FBS_SRC_SEEDED ? 1 : ctw;
        if (x.kind == FBS_SRC_COMPACT) {
            if ((rc = check_bits(ctx, x.bits)) != FBS_OK) return rc;
            words = compact_words(ctx->p.n, x.bits);
            p.W_in = std::max(p.W_in, words);
            p.compact_in.push_back((uint32_t)i);
        }
        if (x.kind == FBS_SRC_SEEDED) {
            if ((rc = check_seeded_streams(ctx, x.nonce0, T)) != FBS_OK) return rc;
            p.any_seeded = true;
        }
        if (x.kind == FBS_SRC_FULL && x.refresh) p.full_refresh.push_back((uint32_t)i);
        p.host_cts |= x.kind != FBS_SRC_SEEDED;
        if (T > SIZE_MAX / 8 / words) return set_error(ctx, FBS_E_INVALID, who + "T * words overflow");
    }
    if (T > SIZE_MAX / 8 / std::max<size_t>(1, n_out) / std::max(ctw, p.W_out)) return set_error(ctx, FBS_E_INVALID, "n_outputs * T words overflow");
    p.n_in_links = p.links.size();
    for (size_t o = 0; out_state && o < n_out; o++) {
        const int64_t w = prog->out_slot[o];
        p.links.push_back(WireLink{out_state->d + o * T * ctw, nullptr, nullptr, w >= 0 ? 0 : trivial_body(ctx, w), w >= 0 ? (uint64_t)w : WIRE_NO_SLOT});
    }
    for (uint32_t i : p.compact_in) p.refresh_slot.push_back(prog->in_slot[i]);
    for (uint32_t i : p.full_refresh) p.refresh_slot.push_back(prog->in_slot[i]);
    p.wait = !out_state || p.host_cts;
    return FBS_OK;
}

// the scratch of a planned call: the chunk and its wire slots (the packed staging of compact inputs and outputs counted in its
// budget), the message rows, the staging, the refresh slots and the identity table, the links, the event of the no-wait path
static int reserve_sources(fbs_ctx *ctx, SourcePlan &p) {
    const fbs_prog *prog = p.prog;
    const size_t W_stage = std::max(p.W_in, p.W_out), rows_per_sample = std::max(1u, prog->max_sources);
    int rc;
    if ((rc = reserve_wires(ctx, prog, p.T, &p.Tc, rows_per_sample * W_stage * 8)) != FBS_OK) return rc;
    if ((p.any_seeded || !p.msgs.empty()) && (rc = ensure_io_msgs(ctx, prog->n_inputs * p.Tc)) != FBS_OK) return rc;
    p.cap_rows = rows_per_sample * p.Tc;   // (ensure_ms has made d_ms at least this long)
    if (W_stage && (rc = grow(ctx, ctx->d_compact, ctx->compact_capacity, p.cap_rows * W_stage, 8, true)) != FBS_OK) return rc;
    if (!p.refresh_slot.empty()) {
        fbs_tvset *made = nullptr;
        if ((rc = identity_tv(ctx, &made)) != FBS_OK) return rc;
        p.tv = made;
    }
    // the refresh slots, then the sample maps of the call [mapped inputs][T]
    if (p.T > (SIZE_MAX / 4 - p.refresh_slot.size()) / std::max<size_t>(1, p.mapped.size())) return set_error(ctx, FBS_E_INVALID, "the sample maps overflow");
    const size_t idx_words = p.refresh_slot.size() + p.mapped.size() * p.T;
    if (idx_words && (rc = ensure_idx(ctx, idx_words)) != FBS_OK) return rc;
    for (size_t j = 0; j < p.mapped.size(); j++) p.links[p.mapped[j].link].index = ctx->d_idx + p.refresh_slot.size() + j * p.T;
    if (p.out_bits) p.cs = compact_store_for(ctx, prog, p.out_bits, p.Tc);
    for (const SourcePlan::At &m : p.msgs) p.links[m.link].msgs = ctx->d_io_msgs + (size_t)m.input * p.Tc;
    if (!p.links.empty() && (rc = grow(ctx, ctx->d_links, ctx->links_capacity, std::max<size_t>(p.links.size(), 1 << 12), sizeof(WireLink), false)) != FBS_OK)
        return rc;
    if (!p.wait && !ctx->inputs_event) FBS_HIP(ctx, hipEventCreateWithFlags(&ctx->inputs_event, hipEventDisableTiming));
    return FBS_OK;
}

// -- the load stage of a chunk, step by step --
// with the first chunk (after eval_chunks's scratch_wait): the refresh slots, the links, the sample maps
static int upload_lists(fbs_ctx *ctx, const SourcePlan &p, const Chunk &c) {
    if (c.s0 != 0) return FBS_OK;
    if (!p.refresh_slot.empty())
        FBS_HIP(ctx, hipMemcpyAsync(ctx->d_idx, p.refresh_slot.data(), p.refresh_slot.size() * 4, hipMemcpyHostToDevice, c.s));
    if (!p.links.empty())
        FBS_HIP(ctx, hipMemcpyAsync(ctx->d_links, p.links.data(), p.links.size() * sizeof(WireLink), hipMemcpyHostToDevice, c.s));
    for (const SourcePlan::At &m : p.mapped)   // the whole map of every mapped input, once a call: the chunks slice it
        FBS_HIP(ctx, hipMemcpyAsync(const_cast<uint32_t *>(p.links[m.link].index), p.maps[m.input].index, p.T * 4, hipMemcpyHostToDevice, c.s));
    return FBS_OK;
}

// the end of the run of inputs that starts at i0: every later one, below n, `joins` it
template <class Joins>
static size_t run_end(size_t i0, size_t n, Joins joins) {
    size_t i1 = i0 + 1;
    while (i1 < n && joins(i1)) i1++;
    return i1;
}

// the chunk's words of inputs [j0, j1), one word a sample in host arrays, into rows j0 .. of the message scratch: one 2D copy per
// stretch of inputs whose arrays lie T words apart
static int upload_rows(fbs_ctx *ctx, const SourcePlan &p, const Chunk &c, size_t j0, size_t j1) {
    const fbs_input_src *src = p.src;
    for (size_t j; j0 < j1; j0 = j) {
        j = run_end(j0, j1, [&](size_t i) { return src[i].data == src[i - 1].data + p.T; });
        FBS_HIP(ctx, hipMemcpy2DAsync(ctx->d_io_msgs + j0 * c.Tc, c.Tc * 8, src[j0].data + c.s0, p.T * 8, c.tc * 8, j - j0, hipMemcpyHostToDevice, c.s));
    }
    return FBS_OK;
}

// inputs that are rows of states, read as they are or through a sample map, and plaintext inputs: the plaintext messages of the
// chunk (8 bytes a sample, nothing for a broadcast), then one launch that moves every row and writes every trivial ciphertext
static int load_links(fbs_ctx *ctx, const SourcePlan &p, const Chunk &c) {
    const size_t n_in = p.prog->n_inputs;
    for (size_t j0 = 0, j1; j0 < n_in; j0 = j1) {   // the messages of the chunk, by stretches of inputs that bring one a sample
        j1 = run_end(j0, n_in, [&](size_t i) { return p.per_sample(j0) && p.per_sample(i); });
        if (!p.per_sample(j0)) continue;
        if (int rc = upload_rows(ctx, p, c, j0, j1)) return rc;
    }
    return dev_wire_load(ctx, WireCopy{ctx->d_links, p.n_in_links, ctx->d_wires, c.Tc, c.s0, c.tc, ctx->D, 2 * ctx->delta_half}, c.s);
}

static int copy_full(fbs_ctx *ctx, const SourcePlan &p, const Chunk &c) {
    const size_t ctw = ctx->D + 1;
    for (size_t i = 0; i < p.prog->n_inputs; i++)
        if (p.from(i, FBS_SRC_FULL))
            FBS_HIP(ctx, hipMemcpyAsync(ctx->d_wires + (size_t)p.prog->in_slot[i] * c.Tc * ctw, p.src[i].data + c.s0 * ctw, c.tc * ctw * 8,
                                        hipMemcpyHostToDevice, c.s));
    return FBS_OK;
}

// runs of seeded inputs whose streams step by T, nonce0 + r T + s over the run's rows r: one expansion each
static int expand_seeded(fbs_ctx *ctx, const SourcePlan &p, const Chunk &c) {
    const size_t n_in = p.prog->n_inputs;
    const fbs_input_src *src = p.src;
    auto seeded = [&](size_t i) { return p.from(i, FBS_SRC_SEEDED); };
    for (size_t i0 = 0, i1; i0 < n_in; i0 = i1) {
        i1 = run_end(i0, n_in, [&](size_t i) { return seeded(i0) && seeded(i) && src[i].nonce0 == src[i - 1].nonce0 + p.T; });
        if (!seeded(i0)) continue;
        if (int rc = upload_rows(ctx, p, c, i0, i1)) return rc;
        IoView v{ctx->d_io_msgs + i0 * c.Tc, c.Tc, ctx->d_wires, p.prog->d_in_slot + i0, c.Tc, i1 - i0, c.tc};
        if (int rc = dev_expand_seeded(ctx, v, src[i0].nonce0 + c.s0, p.T, c.s)) return rc;
    }
    return FBS_OK;
}

// the refresh of `ng` input slots (d_slot [ng], device) of a chunk whose rows d_ms [ng][tc][n + 1] hold already: a blind rotation
// through the identity table written back into the same slots
static int refresh_slots(fbs_ctx *ctx, const fbs_tvset *tv, const uint32_t *d_slot, size_t ng, const Chunk &c) {
    return dev_blind_rotate(ctx, tv, slots_view(ctx->d_wires, ctx->d_wires, d_slot, ng, c.Tc, c.tc), ctx->d_ms, c.s);
}

// compact inputs, in groups whose rows fit the modulus-switch scratch: staged, unpacked into the scratch, refreshed
static int refresh_compact(fbs_ctx *ctx, const SourcePlan &p, const Chunk &c) {
    const size_t group = std::max<size_t>(1, p.cap_rows / c.tc), n1 = ctx->p.n + 1;
    for (size_t g0 = 0; g0 < p.compact_in.size(); g0 += group) {
        const size_t ng = std::min(group, p.compact_in.size() - g0);
        size_t staged = 0;
        for (size_t j = 0; j < ng; j++) {
            const fbs_input_src &x = p.src[p.compact_in[g0 + j]];
            const size_t W = compact_words(ctx->p.n, x.bits);
            FBS_HIP(ctx, hipMemcpyAsync(ctx->d_compact + staged, x.data + c.s0 * W, c.tc * W * 8, hipMemcpyHostToDevice, c.s));
            if (int rc = dev_compact_unpack(ctx, ctx->d_compact + staged, c.tc, x.bits, ctx->d_ms + j * c.tc * n1, c.s)) return rc;
            staged += c.tc * W;
        }
        if (int rc = refresh_slots(ctx, p.tv, ctx->d_idx + g0, ng, c)) return rc;
    }
    return FBS_OK;
}

// full and resident inputs marked `refresh`, in the same groups: key switch and modulus switch, then the refresh in place
static int refresh_full(fbs_ctx *ctx, const SourcePlan &p, const Chunk &c) {
    const size_t group = std::max<size_t>(1, p.cap_rows / c.tc);
    for (size_t g0 = 0; g0 < p.full_refresh.size(); g0 += group) {
        const size_t ng = std::min(group, p.full_refresh.size() - g0);
        const uint32_t *d_slot = ctx->d_idx + p.compact_in.size() + g0;
        const GateView gv = slots_view(ctx->d_wires, nullptr, d_slot, ng, c.Tc, c.tc);
        if (int rc = dev_keyswitch(ctx, gv, ctx->d_ms, ctx->p.log_n_poly + 1, c.s)) return rc;
        if (int rc = refresh_slots(ctx, p.tv, d_slot, ng, c)) return rc;
    }
    return FBS_OK;
}

static int eval_sources(fbs_ctx *ctx, fbs_prog *prog, const fbs_input_src *src, const fbs_resident_src *res, const fbs_sample_map *maps,
                        size_t T, uint32_t out_bits, uint64_t *out, fbs_state *out_state) {
    int rc = check_prog(ctx, prog);
    if (rc != FBS_OK) return rc;
    SourcePlan p;
    if ((rc = plan_sources(ctx, prog, src, res, maps, T, out_bits, out, out_state, p)) != FBS_OK || T == 0) return rc;
    if ((rc = reserve_sources(ctx, p)) != FBS_OK) return rc;
    hipStream_t s = ctx->stream;
    const size_t Tc = p.Tc;
    auto load = [&](size_t s0, size_t tc) {
        const Chunk c{Tc, s0, tc, s};
        int rc;
        if ((rc = upload_lists(ctx, p, c)) || (rc = load_links(ctx, p, c)) || (rc = copy_full(ctx, p, c)) || (rc = expand_seeded(ctx, p, c)) ||
            (rc = refresh_compact(ctx, p, c)) || (rc = refresh_full(ctx, p, c)))
            return rc;
        if (!p.wait && s0 + tc == T) FBS_HIP(ctx, hipEventRecord(ctx->inputs_event, s));   // every array of the caller has been queued
        return FBS_OK;
    };
    auto store = [&](size_t s0, size_t tc) {
        if (out_state) return dev_wire_store(ctx, WireCopy{ctx->d_links + p.n_in_links, prog->n_outputs, ctx->d_wires, Tc, s0, tc, ctx->D, 0}, s);
        return out_bits ? store_compact(ctx, prog, p.cs, out, T, Tc, s0, tc, s) : store_host_cts(ctx, prog, out, T, Tc, s0, tc, s);
    };
    rc = eval_chunks(ctx, prog, T, Tc, s, p.wait, load, store);
    // the links, sample maps, refresh slots, seeded bodies and plaintext messages live in pageable memory of this call or its caller: read before it returns.
    // A call that failed part way may have queued copies from them without reaching the event: it waits for the stream instead.
    if (!p.wait && rc == FBS_OK) FBS_HIP(ctx, hipEventSynchronize(ctx->inputs_event));
    if (!p.wait && rc != FBS_OK) (void)hipStreamSynchronize(s);
    return rc;
}

// The host-buffer entries are eval_sources over n_inputs sources of one kind, input i at data + i * stride words and, seeded, on
// streams nonce0 + i T: one run of n_inputs rows and one 2D copy for seeded bodies, one copy per input for full ciphertexts.
static int eval_uniform(fbs_ctx *ctx, fbs_prog *prog, uint32_t kind, const uint64_t *data, size_t stride, uint64_t nonce0, size_t T,
                        uint32_t out_bits, uint64_t *out) {
    std::vector<fbs_input_src> src(prog->n_inputs);
    for (size_t i = 0; i < src.size(); i++) src[i] = fbs_input_src{kind, 0, 0, kind == FBS_SRC_SEEDED ? nonce0 + i * T : 0, data + i * stride};
    return eval_sources(ctx, prog, src.data(), nullptr, nullptr, T, out_bits, out, nullptr);
}

extern "C" {

// ciphertexts in device memory, ciphertexts out: its own load and store, nothing but launches on `stream`
int fbs_eval_dev(fbs_ctx *ctx, fbs_prog *prog, const uint64_t *d_in, size_t T, uint64_t *d_out, void *stream) try {
    int rc = check_eval(ctx, prog, d_in, T, d_out);
    if (rc != FBS_OK || T == 0) return rc;
    hipStream_t s = pick(ctx, stream);
    const size_t ctw = ctx->D + 1;
    size_t Tc = 0;
    if ((rc = reserve_wires(ctx, prog, T, &Tc)) != FBS_OK) return rc;
    auto load = [&](size_t s0, size_t tc) {   // ciphertexts [n_inputs][T][D + 1] -> the input slots
        for (uint32_t i = 0; i < prog->n_inputs; i++)
            FBS_HIP(ctx, hipMemcpyAsync(ctx->d_wires + (size_t)prog->in_slot[i] * Tc * ctw, d_in + ((size_t)i * T + s0) * ctw, tc * ctw * 8,
                                        hipMemcpyDeviceToDevice, s));
        return FBS_OK;
    };
    auto store = [&](size_t s0, size_t tc) {
        for (uint32_t o = 0; o < prog->n_outputs; o++) {
            const int64_t w = prog->out_slot[o];
            uint64_t *dst = d_out + ((size_t)o * T + s0) * ctw;
            if (int rc = dev_copy_out(ctx, ctx->d_wires, Tc, 0, tc, w, w < 0 ? trivial_body(ctx, w) : 0, dst, s)) return rc;
        }
        return FBS_OK;
    };
    return eval_chunks(ctx, prog, T, Tc, s, false, load, store);
} FBS_API_CATCH(ctx)

int fbs_eval(fbs_ctx *ctx, fbs_prog *prog, const uint64_t *in_cts, size_t T, uint64_t *out_cts) try {
    int rc = check_eval(ctx, prog, in_cts, T, out_cts);
    if (rc != FBS_OK || T == 0) return rc;
    return eval_uniform(ctx, prog, FBS_SRC_FULL, in_cts, T * (ctx->D + 1), 0, T, 0, out_cts);
} FBS_API_CATCH(ctx)

// Messages in, messages out: fbs_eval with the inputs encrypted on the device straight into their wire slots and the output
// slots decrypted there (the same chunks, scratch ordering and checks); only int64 messages cross the bus.
int fbs_eval_messages(fbs_ctx *ctx, fbs_prog *prog, const int64_t *msgs, size_t T, int fresh, uint64_t *nonce0, int64_t *out_msgs) try {
    int rc = check_eval(ctx, prog, msgs, T, out_msgs);
    if (rc != FBS_OK) return rc;
    if (!fresh && !nonce0) return set_error(ctx, FBS_E_INVALID, "null argument");
    if (ctx->eval_only) return set_error(ctx, FBS_E_STATE, EVAL_ONLY);
    if (T == 0) return FBS_OK;
    const size_t n_in = prog->n_inputs, n_out = prog->n_outputs;
    if (T > SIZE_MAX / 8 / std::max<size_t>(1, n_in + n_out) || (rc = check_ct_words(ctx, T * std::max<size_t>(1, n_in))))
        return set_error(ctx, FBS_E_INVALID, "n_inputs * T ciphertexts overflow");
    const size_t streams = n_in * T;
    if (!fresh && (rc = check_nonces(ctx, *nonce0, streams))) return rc;
    hipStream_t s = ctx->stream;
    size_t Tc = 0;
    if ((rc = reserve_wires(ctx, prog, T, &Tc)) != FBS_OK) return rc;
    if ((rc = ensure_io_msgs(ctx, (n_in + n_out) * Tc)) != FBS_OK) return rc;
    uint64_t first = fresh ? 0 : *nonce0;
    if (fresh) {
        if ((rc = reserve_fresh(ctx, streams, &first))) return rc;
        if (nonce0) *nonce0 = first;
    }
    // what fbs_decrypt makes of the trivial ciphertext fbs_eval returns for a constant output
    std::vector<int64_t> const_msg(n_out, 0);
    {
        std::vector<uint64_t> triv(ctx->D + 1, 0);
        for (size_t o = 0; o < n_out; o++)
            if (prog->out_slot[o] < 0) {
                triv[ctx->D] = trivial_body(ctx, prog->out_slot[o]);
                host_decrypt(ctx, triv.data(), 1, &const_msg[o]);
            }
    }
    int64_t *d_in_msgs = ctx->d_io_msgs, *d_out_msgs = ctx->d_io_msgs + n_in * Tc;
    auto load = [&](size_t s0, size_t tc) {
        if (!n_in) return FBS_OK;
        FBS_HIP(ctx, hipMemcpy2DAsync(d_in_msgs, Tc * 8, msgs + s0, T * 8, tc * 8, n_in, hipMemcpyHostToDevice, s));
        return dev_encrypt(ctx, IoView{d_in_msgs, Tc, ctx->d_wires, prog->d_in_slot, Tc, n_in, tc}, first + s0, T, s);
    };
    auto store = [&](size_t s0, size_t tc) {
        if (!n_out) return FBS_OK;
        if (int rc = dev_decrypt(ctx, IoView{d_out_msgs, Tc, ctx->d_wires, prog->d_out_slot, Tc, n_out, tc}, s)) return rc;
        FBS_HIP(ctx, hipMemcpy2DAsync(out_msgs + s0, T * 8, d_out_msgs, Tc * 8, tc * 8, n_out, hipMemcpyDeviceToHost, s));
        return FBS_OK;
    };
    auto post = [&](size_t s0, size_t tc) {
        for (size_t o = 0; o < n_out; o++)
            if (prog->out_slot[o] < 0) std::fill(out_msgs + o * T + s0, out_msgs + o * T + s0 + tc, const_msg[o]);
        return FBS_OK;
    };
    return eval_chunks(ctx, prog, T, Tc, s, true, load, store, post);
} FBS_API_CATCH(ctx)

// Seeded inputs: fbs_eval with the bodies copied to the device and expanded there straight into their wire slots (the chunks,
// scratch ordering and outputs of fbs_eval); needs no secret.  The bodies use fbs_eval_messages's message scratch.
int fbs_eval_seeded(fbs_ctx *ctx, fbs_prog *prog, const uint64_t *bodies, size_t T, uint64_t nonce0, uint64_t *out_cts) try {
    int rc = check_eval(ctx, prog, bodies, T, out_cts);
    if (rc != FBS_OK || T == 0) return rc;
    const size_t n_in = prog->n_inputs, n_out = prog->n_outputs, ctw = ctx->D + 1;
    if (T > SIZE_MAX / 8 / std::max<size_t>(1, std::max(n_in, n_out)) / ctw)
        return set_error(ctx, FBS_E_INVALID, "n_inputs * T ciphertexts overflow");
    if ((rc = check_seeded_streams(ctx, nonce0, n_in * T))) return rc;   // (before any nonce0 + i T is formed: none wraps)
    return eval_uniform(ctx, prog, FBS_SRC_SEEDED, bodies, T, nonce0, T, 0, out_cts);
} FBS_API_CATCH(ctx)

// ---- compact outputs: key switch to the small key, rounding to Z_(2^bits), bit packing (fbs_compact.hpp) --------------------
// (no secret needed: runs on evaluation-only contexts)
int fbs_compact_dev(fbs_ctx *ctx, const uint64_t *d_cts, size_t count, uint32_t bits, uint64_t *d_words, void *stream) try {
    if (int rc = io_prologue(ctx, d_cts, d_words, count, IO_CT_WORDS, nullptr)) return rc;
    if (int rc = check_bits(ctx, bits)) return rc;
    if (int rc = check_compact_words(ctx, count, bits)) return rc;
    if (count == 0) return FBS_OK;
    FBS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t ctw = ctx->D + 1, W = compact_words(ctx->p.n, bits);
    hipStream_t s = pick(ctx, stream);
    return ms_passes(ctx, count, s, [&](size_t f0, size_t rows) {
        const GateView gv = batch_view(d_cts + f0 * ctw, nullptr, nullptr, rows);
        if (int rc = dev_keyswitch(ctx, gv, ctx->d_ms, bits, s)) return rc;
        return dev_compact_pack(ctx, ctx->d_ms, rows, bits, d_words + f0 * W, s);
    });
} FBS_API_CATCH(ctx)

// fbs_eval_seeded with the compact store stage
int fbs_eval_seeded_compact(fbs_ctx *ctx, fbs_prog *prog, const uint64_t *bodies, size_t T, uint64_t nonce0, uint32_t bits,
                            uint64_t *out_words) try {
    int rc = check_eval(ctx, prog, bodies, T, out_words);
    if (rc != FBS_OK) return rc;
    if ((rc = check_bits(ctx, bits)) != FBS_OK || T == 0) return rc;
    const size_t n_in = prog->n_inputs, n_out = prog->n_outputs, ctw = ctx->D + 1, W = compact_words(ctx->p.n, bits);
    if (T > SIZE_MAX / 8 / std::max<size_t>(1, std::max(n_in, n_out)) / std::max(ctw, W))
        return set_error(ctx, FBS_E_INVALID, "n_inputs * T ciphertexts overflow");
    if ((rc = check_seeded_streams(ctx, nonce0, n_in * T))) return rc;
    return eval_uniform(ctx, prog, FBS_SRC_SEEDED, bodies, T, nonce0, T, bits, out_words);
} FBS_API_CATCH(ctx)

int fbs_eval_sources(fbs_ctx *ctx, fbs_prog *prog, const fbs_input_src *src, size_t T, uint32_t out_bits, uint64_t *out) try {
    if (int rc = check_eval(ctx, prog, src, T, out)) return rc;
    return eval_sources(ctx, prog, src, nullptr, nullptr, T, out_bits, out, nullptr);
} FBS_API_CATCH(ctx)

// fbs_eval_resident with sample maps on its resident inputs (fbs_state.hip, "sample-axis operations")
int fbs_eval_resident_mapped(fbs_ctx *ctx, fbs_prog *prog, const fbs_input_src *src, const fbs_resident_src *res, const fbs_sample_map *maps,
                             size_t T, uint32_t out_bits, uint64_t *out_host, fbs_state *out_state) try {
    if (!ctx) return FBS_E_INVALID;
    if ((out_host != nullptr) == (out_state != nullptr))
        return set_error(ctx, FBS_E_INVALID, "exactly one of out_host and out_state takes the outputs");
    return eval_sources(ctx, prog, src, res, maps, T, out_bits, out_host, out_state);
} FBS_API_CATCH(ctx)

int fbs_eval_resident(fbs_ctx *ctx, fbs_prog *prog, const fbs_input_src *src, const fbs_resident_src *res, size_t T, uint32_t out_bits,
                      uint64_t *out_host, fbs_state *out_state) try {
    return fbs_eval_resident_mapped(ctx, prog, src, res, nullptr, T, out_bits, out_host, out_state);
} FBS_API_CATCH(ctx)

}   // extern "C"

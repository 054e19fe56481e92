// jst_normalize.hpp -- projected pan-genome alignments with every gap run at its leftmost equivalent place
// (spm_hip_jst_ref_alns_normalize; contract in spm_hip.h, scheme in DESIGN.md 4.6c).  gfx950.  Unit: jst_ref.hip.  It reads
// and makes a spm_jst_ref_alns (jst_handles.hpp).
//
// Records that share a transcript slot share needle, reference range and words, so the rule is applied once per distinct slot
// of the source pool and gathered:
//   (the slot stage of transcript_slots.hpp: a representative record and a number for every distinct slot, in pool order)
//   jst_norm_walk_kernel     one lane per slot: jst_normalize_walk of jst_normalize_core.hpp with the slot's slice of a scratch
//                            buffer of twice the source pool as its stack, [2 cigar_off, 2 (cigar_off + cigar_len)); the words
//                            of the result, whether they differ from the source's, steps, joins, pinned runs
//   (hipcub exclusive sum of the word counts, 64 bits; slot_total_kernel)
//   jst_norm_gather_kernel   one lane per record i: its own record + offset and length of its slot -> spm_jst_ref_aln i; a
//                            record that disagrees with the representative of its slot is counted
//   (the one read-back that sizes the pool: {slots, errors, words, changed, steps, joined, pinned})
//   jst_norm_compact_kernel  one lane per slot: its slice -> its place in the pool
// The scratch is laid out with scratch_layout.hpp; the launches, the sums, the read-back and the events are
// device_order.hpp's; what makes a record unusable (ref_aln_unusable), the slot clamp and the total kernel are
// transcript_slots.hpp's.  Every needle, reference and pool index is tested against its size before it is read.
#pragma once

#include "internal.hpp"
#include "device_order.hpp"
#include "jst_handles.hpp"
#include "jst_normalize_core.hpp"
#include "scratch_layout.hpp"
#include "transcript_slots.hpp"
#include "wave.hpp"

static_assert(SPM_CIGAR_INS == spm_hip::kNormIns && SPM_CIGAR_DEL == spm_hip::kNormDel && SPM_CIGAR_EQ == spm_hip::kNormEq &&
                  SPM_CIGAR_X == spm_hip::kNormX, "the core header's op values are the ABI's");

namespace spm_hip
{

enum { kNormCntSlots = 0, kNormCntBad, kNormCntWords, kNormCntChanged, kNormCntSteps, kNormCntJoined, kNormCntPinned, kNormCnts };
static_assert(kNormCntSlots == kSlotCntSlots && kNormCntBad == kSlotCntBad, "the slot stage writes the first two counters");
static_assert(kNormCnts <= kCntBlock, "the read-back lands in the context's counter block");

struct jst_normalize_params
{
    const spm_jst_ref_aln *recs;     // the source's device view
    uint32_t n;
    const uint32_t *ops;             // the source's pool
    uint64_t n_ops;
    const uint8_t *ref;              // the reference's ranks
    uint64_t n_ref;
    const uint8_t *ranks;            // the needles' symbols, back to back ...
    const uint32_t *offsets;         // ... and where each starts
    const int32_t *m;
    uint32_t n_patterns;
    uint32_t cap;                    // slots the per-slot tables hold: min(n, n_ops)
    uint32_t *rep;                   // [n_ops] smallest record index whose transcript starts at this word, or none
    uint32_t *sid;                   // [n_ops] exclusive sum of rep != none: the slot's number
    uint32_t *slot_rec;              // [cap] representative record of slot s
    uint32_t *stack;                 // [2 * n_ops] slot with transcript [off, off + len) works in [2 off, 2 (off + len))
    uint32_t *slot_words;            // [cap] words of the normalised transcript
    const unsigned long long *slot_off; // [cap] exclusive sum of slot_words
    unsigned long long *counts;      // kNormCnt*
    spm_jst_ref_aln *out;            // [n]
    slot_tables slots() const { return slot_tables{rep, sid, slot_rec, n_ops, cap, counts}; } // (what the slot stage takes)
};

// a slot's slice of the stack buffer
struct jnorm_slice
{
    uint32_t *w;
    uint64_t n;
    __device__ __forceinline__ uint64_t cap() const { return n; }
    __device__ __forceinline__ uint32_t get(uint64_t k) const { return w[k]; }
    __device__ __forceinline__ void put(uint64_t k, uint32_t v) { w[k] = v; }
};

__global__ __launch_bounds__(256) void jst_norm_walk_kernel(const jst_normalize_params P)
{
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    bool bad = false, changed = false;
    unsigned long long steps = 0, joined = 0, pinned = 0;
    if (s < slot_count(P.counts, P.cap)) {
        const uint32_t ri = P.slot_rec[s];
        spm_jst_ref_aln a{};
        bad = ri >= P.n;
        if (!bad) {
            a = P.recs[ri];
            bad = ref_aln_unusable(P, a);
        }
        const int32_t m = bad ? 0 : P.m[a.pattern];
        bad = bad || m <= 0;
        uint32_t nw = 0;
        if (!bad) {
            jnorm_slice S{P.stack + 2 * (uint64_t)a.cigar_off, 2 * (uint64_t)a.cigar_len};
            jst_norm_result R;
            bad = !jst_normalize_walk(P.ops + a.cigar_off, a.cigar_len, P.ranks + P.offsets[a.pattern], (uint32_t)m, P.ref,
                                      P.n_ref, a.ref_begin, a.ref_end, S, R) || R.n_words > S.n;
            if (!bad) {
                nw = (uint32_t)R.n_words;
                steps = R.n_steps;
                joined = R.n_joined;
                pinned = R.n_pinned;
                changed = nw != a.cigar_len;
                for (uint32_t w = 0; !changed && w < nw; ++w)
                    changed = S.w[w] != P.ops[a.cigar_off + w];
            }
        }
        P.slot_words[s] = nw;
    }
    count_flagged(&P.counts[kNormCntBad], bad);
    count_flagged(&P.counts[kNormCntChanged], changed);
    if (steps)
        atomicAdd(&P.counts[kNormCntSteps], steps);
    if (joined)
        atomicAdd(&P.counts[kNormCntJoined], joined);
    if (pinned)
        atomicAdd(&P.counts[kNormCntPinned], pinned);
}

__global__ __launch_bounds__(256) void jst_norm_gather_kernel(const jst_normalize_params P)
{
    const unsigned long long i = blockIdx.x * 256ull + threadIdx.x;
    bool bad = false;
    if (i < P.n) {
        spm_jst_ref_aln o = P.recs[i];
        bad = true;
        if (!ref_aln_unusable(P, o)) {
            const uint32_t s = P.sid[o.cigar_off];
            const uint32_t r = s < P.cap ? P.slot_rec[s] : kSlotNone;
            if (r < P.n) {
                // a record must say what the representative of its slot says: the rule was applied to that one
                const spm_jst_ref_aln q = P.recs[r];
                bad = q.cigar_off != o.cigar_off || q.cigar_len != o.cigar_len || q.pattern != o.pattern ||
                      q.ref_begin != o.ref_begin || q.ref_end != o.ref_end || P.slot_off[s] > 0xFFFFFFFFull;
                if (!bad) {
                    o.cigar_off = (uint32_t)P.slot_off[s];
                    o.cigar_len = P.slot_words[s];
                }
            }
        }
        if (bad)
            o.cigar_off = o.cigar_len = 0;
        P.out[i] = o;
    }
    count_flagged(&P.counts[kNormCntBad], bad);
}

// pool_words: the size of out_ops, which the host allocated from the total the read-back brought
__global__ __launch_bounds__(256) void jst_norm_compact_kernel(const jst_normalize_params P, uint32_t *out_ops, uint64_t pool_words)
{
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    bool bad = false;
    if (s < slot_count(P.counts, P.cap)) {
        const uint32_t ri = P.slot_rec[s];
        const unsigned long long off = P.slot_off[s];
        const uint32_t nw = P.slot_words[s];
        bad = ri >= P.n || off + nw > pool_words;
        if (!bad) {
            const spm_jst_ref_aln a = P.recs[ri];
            bad = ref_aln_unusable(P, a) || nw > 2 * (uint64_t)a.cigar_len;
            if (!bad) {
                const uint32_t *src = P.stack + 2 * (uint64_t)a.cigar_off;
                for (uint32_t w = 0; w < nw; ++w)
                    out_ops[off + w] = src[w];
            }
        }
    }
    count_flagged(&P.counts[kNormCntBad], bad);
}

} // namespace spm_hip

extern "C" int spm_hip_jst_ref_alns_normalize(spm_jst_ref_alns *a, uint32_t flags, spm_jst_ref_alns **out)
{
    using namespace spm_hip;
    if (!a || !out)
        return SPM_E_INVALID;
    spm_ctx *ctx = a->ctx;
    const auto t_call = clk::now();
    if (flags) {
        SPM_SET_ERR(ctx, "spm_hip_jst_ref_alns_normalize: unknown flag bits 0x%x", flags);
        return SPM_E_INVALID;
    }
    spm_jst *J = a->jst;
    const spm_patterns *ps = a->patterns;
    if (!J || !ps || !J->ref) {
        SPM_SET_ERR(ctx, "spm_hip_jst_ref_alns_normalize: these alignments name no tree");
        return SPM_E_INVALID;
    }
    const uint64_t n = a->n, n_src_ops = a->n_ops;
    if (n > 0xFFFFFFFFull) {
        SPM_SET_ERR(ctx, "spm_hip_jst_ref_alns_normalize: more than 2^32 - 1 records");
        return SPM_E_UNSUPPORTED;
    }
    SPM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    std::unique_ptr<spm_jst_ref_alns, void (*)(spm_jst_ref_alns *)> R(new spm_jst_ref_alns, spm_hip_jst_ref_alns_destroy);
    R->ctx = ctx;
    R->n = n;
    R->n_patterns = a->n_patterns;
    R->n_ref = a->n_ref;
    R->jst = J;
    R->patterns = ps;
    R->normalized = true;
    spm_jst_normalize_stats &S = R->norm_stats;
    S.n_alns = n;
    S.n_ops_in = n_src_ops;
    hipStream_t st = ctx->stream;
    float ms_slots = 0, ms_walk = 0, ms_offsets = 0, ms_gather = 0, ms_compact = 0;
    if (n) {
        if (n_src_ops == 0 || !a->d_ops || !a->d_recs || a->host.size() != n) {
            SPM_SET_ERR(ctx, "spm_hip_jst_ref_alns_normalize: %llu records but no transcript pool or no host view",
                        (unsigned long long)n);
            return SPM_E_INVALID;
        }
        SPM_TRY(spm_align_tables(ps)); // the needles' ranks on the device (built once per set)
        const uint32_t n32 = (uint32_t)n;
        const uint32_t cap = (uint32_t)std::min<uint64_t>(n, n_src_ops);
        hip_events<7> ev;
        SPM_HIP_CHECK(ctx, ev.create());
        size_t b_flag = 0, b_wide = 0;
        SPM_HIP_CHECK(ctx, slot_stage_tmp_bytes(ctx, n_src_ops, &b_flag));
        SPM_HIP_CHECK(ctx, exclusive_sum_tmp_bytes<unsigned long long>(ctx, counted<unsigned long long>(widen_op{nullptr}), cap,
                                                                       &b_wide));
        const size_t tmp_bytes = std::max(b_flag, b_wide);
        jst_normalize_params P{};
        unsigned long long *d_off = nullptr; // (P.slot_off, writable for the sum)
        uint8_t *d_tmp = nullptr;
        scratch_layout L;
        L.take(P.rep, n_src_ops);
        L.take(P.sid, n_src_ops);
        L.take(P.slot_rec, cap);
        L.take(P.stack, 2 * n_src_ops);
        L.take(P.slot_words, cap);
        L.take(d_off, cap);
        L.take(P.counts, kNormCnts);
        L.take(d_tmp, tmp_bytes);
        SPM_TRY(ensure_scratch(ctx, L.bytes()));
        L.bind(ctx->d_scratch);
        SPM_HIP_CHECK(ctx, hipMalloc(&R->d_recs, n * sizeof(spm_jst_ref_aln)));

        P.recs = a->d_recs;
        P.n = n32;
        P.ops = a->d_ops;
        P.n_ops = n_src_ops;
        P.ref = J->ref->d;
        P.n_ref = J->ref->n;
        P.ranks = ps->d_al_ranks;
        P.offsets = ps->d_al_offsets;
        P.m = ps->d_m;
        P.n_patterns = std::min(ps->n, a->n_patterns);
        P.cap = cap;
        P.slot_off = d_off;
        P.out = R->d_recs;
        // ---- slots: one representative per distinct slot of the source pool, numbered in pool order ----
        SPM_HIP_CHECK(ctx, hipMemsetAsync(P.counts, 0, kNormCnts * 8, st));
        SPM_HIP_CHECK(ctx, hipEventRecord(ev[0], st));
        SPM_HIP_CHECK(ctx, slot_stage_enqueue(ctx, P.recs, n32, P.slots(), ref_aln_unusable_op{{P.n_ops, P.n_patterns, P.n_ref}},
                                              d_tmp, tmp_bytes));
        SPM_HIP_CHECK(ctx, hipEventRecord(ev[1], st));
        // ---- normalise: the rule on every slot, in its slice of the stack buffer ----
        SPM_HIP_CHECK(ctx, hipMemsetAsync(P.slot_words, 0, (size_t)cap * 4, st));
        SPM_HIP_CHECK(ctx, launch_1d(ctx, jst_norm_walk_kernel, cap, P));
        SPM_HIP_CHECK(ctx, hipEventRecord(ev[2], st));
        // ---- offsets: where every slot's words go, and how many there are ----
        SPM_HIP_CHECK(ctx, exclusive_sum(ctx, d_tmp, tmp_bytes, counted<unsigned long long>(widen_op{P.slot_words}), d_off, cap));
        SPM_HIP_CHECK(ctx, launch_1d<64>(ctx, slot_total_kernel, 1, P.counts, cap, P.slot_off, P.slot_words, kNormCntWords));
        SPM_HIP_CHECK(ctx, hipEventRecord(ev[3], st));
        // ---- gather: one record per source record (it needs the offsets, not the pool) ----
        SPM_HIP_CHECK(ctx, launch_1d(ctx, jst_norm_gather_kernel, n, P));
        SPM_HIP_CHECK(ctx, hipEventRecord(ev[4], st));
        // the one read-back that sizes the pool: {slots, errors, words, changed, steps, joined, pinned}
        SPM_HIP_CHECK(ctx, read_counts(ctx, P.counts, kNormCnts));
        unsigned long long *c = ctx->h_counters;
        const unsigned long long n_slots = c[kNormCntSlots], n_bad = c[kNormCntBad], total = c[kNormCntWords];
        if (n_bad || n_slots == 0 || n_slots > cap || total > 2 * n_src_ops) {
            SPM_SET_ERR(ctx, "spm_hip_jst_ref_alns_normalize: %llu records or transcript slots cannot be normalised (a "
                             "transcript outside the pool, words that do not consume exactly their needle and their reference "
                             "range, a range outside the reference, or a record that disagrees with its slot); nothing was "
                             "normalised", n_bad ? n_bad : (unsigned long long)n);
            return SPM_E_INVALID;
        }
        if (total > 0xFFFFFFFFull) { // decided before the compact launch
            SPM_SET_ERR(ctx, "spm_hip_jst_ref_alns_normalize: the normalised CIGAR pool would exceed 2^32 - 1 words");
            return SPM_E_UNSUPPORTED;
        }
        S.n_slots = n_slots;
        S.n_changed = c[kNormCntChanged];
        S.n_steps = c[kNormCntSteps];
        S.n_joined = c[kNormCntJoined];
        S.n_pinned = c[kNormCntPinned];
        R->n_ops = total;
        SPM_HIP_CHECK(ctx, hipMalloc(&R->d_ops, std::max<uint64_t>(total, 1) * 4));
        // ---- compact: the slices into the pool ----
        SPM_HIP_CHECK(ctx, hipEventRecord(ev[5], st));
        SPM_HIP_CHECK(ctx, launch_1d(ctx, jst_norm_compact_kernel, n_slots, P, R->d_ops, total));
        SPM_HIP_CHECK(ctx, hipEventRecord(ev[6], st));
        // ---- the host view: record i of the source's host view through the slot tables ----
        slot_host_map slot(n_src_ops);
        std::vector<uint32_t> words(n_slots);
        std::vector<unsigned long long> woff(n_slots);
        R->host_ops.resize(total);
        SPM_HIP_CHECK(ctx, hipMemcpyAsync(c, P.counts, kNormCnts * 8, hipMemcpyDeviceToHost, st));
        SPM_HIP_CHECK(ctx, slot.download(ctx, P.slots()));
        SPM_HIP_CHECK(ctx, hipMemcpyAsync(words.data(), P.slot_words, n_slots * 4, hipMemcpyDeviceToHost, st));
        SPM_HIP_CHECK(ctx, hipMemcpyAsync(woff.data(), d_off, n_slots * 8, hipMemcpyDeviceToHost, st));
        if (total)
            SPM_HIP_CHECK(ctx, hipMemcpyAsync(R->host_ops.data(), R->d_ops, total * 4, hipMemcpyDeviceToHost, st));
        SPM_HIP_CHECK(ctx, hipStreamSynchronize(st));
        hipEventElapsedTime(&ms_slots, ev[0], ev[1]);
        hipEventElapsedTime(&ms_walk, ev[1], ev[2]);
        hipEventElapsedTime(&ms_offsets, ev[2], ev[3]);
        hipEventElapsedTime(&ms_gather, ev[3], ev[4]);
        hipEventElapsedTime(&ms_compact, ev[5], ev[6]);
        if (c[kNormCntBad]) {
            SPM_SET_ERR(ctx, "spm_hip_jst_ref_alns_normalize: %llu transcript slots came out of the compact stage differently "
                             "from the count", c[kNormCntBad]);
            return SPM_E_INVALID;
        }
        R->host.resize(n);
        for (uint64_t i = 0; i < n; ++i) {
            spm_jst_ref_aln x = a->host[i];
            const uint32_t s = slot.of(x.cigar_off);
            if (s >= n_slots) {
                SPM_SET_ERR(ctx, "spm_hip_jst_ref_alns_normalize: host record %llu names no slot", (unsigned long long)i);
                return SPM_E_INVALID;
            }
            x.cigar_off = (uint32_t)woff[s];
            x.cigar_len = words[s];
            R->host[i] = x;
        }
    }
    S.ms_slots = ms_slots;
    S.ms_normalize = ms_walk;
    S.ms_offsets = ms_offsets;
    S.ms_gather = ms_gather;
    S.ms_compact = ms_compact;
    S.ms_total = ms_slots + ms_walk + ms_offsets + ms_gather + ms_compact;
    S.n_ops = R->n_ops;
    R->stats.n_alns = n; // what spm_hip_jst_ref_alns_stats answers for this handle: the counts, no times
    R->stats.n_projected = S.n_slots;
    R->stats.n_ops = R->n_ops;
    S.ms_host = ms_since(t_call);
    if (spm_trace_on())
        fprintf(stderr, "[spm_hip] jst normalize: %llu records, %llu slots, %llu -> %llu words (%llu changed, %llu steps, %llu "
                        "joins, %llu pinned): slots %.3f ms, normalise %.3f, offsets %.3f, gather %.3f, compact %.3f; %.3f ms in "
                        "all\n", (unsigned long long)n, (unsigned long long)S.n_slots, (unsigned long long)n_src_ops,
                (unsigned long long)R->n_ops, (unsigned long long)S.n_changed, (unsigned long long)S.n_steps,
                (unsigned long long)S.n_joined, (unsigned long long)S.n_pinned, ms_slots, ms_walk, ms_offsets, ms_gather,
                ms_compact, S.ms_host);
    *out = R.release();
    return SPM_OK;
}

extern "C" int spm_hip_jst_ref_alns_normalize_stats(const spm_jst_ref_alns *a, spm_jst_normalize_stats *out)
{
    if (!a || !out)
        return SPM_E_INVALID;
    if (!a->normalized) {
        SPM_SET_ERR(a->ctx, "spm_hip_jst_ref_alns_normalize_stats: these alignments were not made by "
                            "spm_hip_jst_ref_alns_normalize");
        return SPM_E_INVALID;
    }
    *out = a->norm_stats;
    return SPM_OK;
}

// jst_project.hpp -- pan-genome alignments in reference coordinates (spm_hip_jst_alns_project; contract in spm_hip.h, scheme
// in DESIGN.md 4.6).  gfx950.  Unit: jst_ref.hip.  It reads spm_jst and spm_jst_alns (jst_handles.hpp), walks with
// jst_walk_core.hpp's jst_first_ref and begins with the slot stage of transcript_slots.hpp.
//
// Records that share a transcript slot share a context: they carry the same alleles over it and lie on the same reference
// positions.  So the projection is computed once per distinct slot of the source pool and gathered:
//   (the slot stage of transcript_slots.hpp: a representative record and a number for every distinct slot, in pool order)
//   jst_proj_count_kernel    one lane per slot: the block of its haplotype that holds `begin` (binary search down column h of
//                            hap_start), the journal walked from jst_first_ref / a_lo up to begin, then jst_project_compose
//                            with a counting sink: words, ref_begin, ref_end, ref_score
//   (hipcub exclusive sum of the word counts, 64 bits; slot_total_kernel; the one read-back that sizes the pool)
//   jst_proj_emit_kernel     the same walk with a writing sink
//   jst_proj_gather_kernel   one lane per record i: its own record + the result of its slot -> spm_jst_ref_aln i
// The scratch is laid out with scratch_layout.hpp; the launches, the sums, the first read-back and the events are
// device_order.hpp's; the slot clamp and the total kernel are transcript_slots.hpp's, the count of the flagged lanes wave.hpp's.
// The walk starts from the tables of the index and runs forward as far as the transcript reaches: it assumes neither that a
// carried deletion ends inside its block nor that begin and end lie in the same block.
#pragma once

#include "internal.hpp"
#include "device_order.hpp"
#include "jst_handles.hpp"
#include "jst_project_core.hpp"
#include "scratch_layout.hpp"
#include "transcript_slots.hpp"
#include "wave.hpp"

static_assert(SPM_CIGAR_INS == spm_hip::kProjIns && SPM_CIGAR_DEL == spm_hip::kProjDel && SPM_CIGAR_EQ == spm_hip::kProjEq &&
                  SPM_CIGAR_X == spm_hip::kProjX, "the core header's op values are the ABI's");

namespace spm_hip
{

enum { kProjCntSlots = 0, kProjCntBad = 1, kProjCntInside = 2, kProjCntChanged = 3, kProjCntWords = 4, kProjCnts = 5 };
static_assert(kProjCntSlots == kSlotCntSlots && kProjCntBad == kSlotCntBad, "the slot stage writes the first two counters");

struct jst_project_params
{
    jst_dev J;                       // allele table, coverage, a_lo, hap_start (all blocks of the reference)
    const spm_jst_aln *recs;         // the source's device view
    uint32_t n;
    const uint32_t *ops;             // the source's pool
    uint64_t n_ops;
    const uint8_t *ranks;            // the needles' symbols, back to back ...
    const uint32_t *offsets;         // ... and where each starts
    const int32_t *m;
    uint32_t n_patterns;
    uint32_t cap;                    // slots the per-slot tables hold: min(n, n_ops)
    uint32_t *rep;                   // [n_ops] smallest record index whose transcript starts at this word, or none
    uint32_t *sid;                   // [n_ops] exclusive sum of rep != none: the slot's number
    uint32_t *slot_rec;              // [cap] representative record of slot s
    unsigned long long *slot_range;  // [2 * cap] ref_begin, ref_end
    uint32_t *slot_words;            // [cap] words of the projected transcript
    int32_t *slot_score;             // [cap] ref_score
    const unsigned long long *slot_off; // [cap] exclusive sum of slot_words
    uint32_t *out_ops;
    unsigned long long *counts;      // kProjCnt*
    spm_jst_ref_aln *out;            // [n]
    slot_tables slots() const { return slot_tables{rep, sid, slot_rec, n_ops, cap, counts}; } // (what the slot stage takes)
};

// what makes a record unusable for the slot stage
struct jproj_unusable
{
    uint64_t n_ops;
    __device__ __forceinline__ bool operator()(const spm_jst_aln &a) const
    {
        return a.cigar_len == 0 || (uint64_t)a.cigar_off + a.cigar_len > n_ops;
    }
};

// The projection of slot s into sink S.  Every table index is tested against its size before it is read; false counts as an
// error of the call, never a fault.
template <class Sink>
__device__ __forceinline__ bool jproj_run(const jst_project_params &P, uint32_t s, Sink &S, jst_proj_result &R, spm_jst_aln &a)
{
    const jst_dev &J = P.J;
    const uint32_t ri = P.slot_rec[s];
    if (ri >= P.n)
        return false;
    a = P.recs[ri];
    const uint32_t h = a.haplotype;
    if (h >= J.n_hap || a.pattern >= P.n_patterns || a.cigar_len == 0 || (uint64_t)a.cigar_off + a.cigar_len > P.n_ops ||
        a.begin > a.end)
        return false;
    const int32_t m = P.m[a.pattern];
    if (m <= 0)
        return false;
    // the largest j in [0, n_blocks] with hap_start[j][h] <= begin (the column is non-decreasing and starts at 0)
    uint64_t lo = 0, hi = J.n_blocks + 1;
    if (J.hap_start[h] > a.begin)
        return false;
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (J.hap_start[mid * J.n_hap + h] <= a.begin)
            lo = mid;
        else
            hi = mid;
    }
    jst_journal_view V;
    V.pos = J.pos;
    V.rlen = J.rlen;
    V.alen = J.alen;
    V.cov = J.cov;
    V.n_alleles = J.n_alleles;
    V.cw = J.cw;
    V.n_hap = J.n_hap;
    V.n_ref = J.n_ref;
    jst_journal_cursor C;
    const uint64_t first_allele = J.a_lo[lo];
    if (first_allele > J.n_alleles)
        return false;
    C.start(V, h, jst_first_ref(J, lo, h), first_allele);
    if (!C.skip(a.begin - J.hap_start[lo * J.n_hap + h]))
        return false;
    return jst_project_compose(C, P.ops + a.cigar_off, a.cigar_len, P.ranks + P.offsets[a.pattern], (uint32_t)m, J.ref, J.n_ref,
                               S, R);
}

__global__ __launch_bounds__(256) void jst_proj_count_kernel(const jst_project_params P)
{
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    const uint32_t n_slots = slot_count(P.counts, P.cap);
    bool bad = false, inside = false;
    if (s < n_slots) {
        jst_proj_count_sink S;
        jst_proj_result R;
        spm_jst_aln a;
        bad = !jproj_run(P, s, S, R, a) || R.n_words > 0xFFFFFFFFull || R.ref_score > 0x7FFFFFFFull;
        inside = !bad && R.inside;
        P.slot_range[2 * (uint64_t)s] = bad ? 0ull : R.ref_begin;
        P.slot_range[2 * (uint64_t)s + 1] = bad ? 0ull : R.ref_end;
        P.slot_words[s] = bad ? 0u : (uint32_t)R.n_words;
        P.slot_score[s] = bad ? 0 : (int32_t)R.ref_score;
    }
    count_flagged(&P.counts[kProjCntBad], bad);
    count_flagged(&P.counts[kProjCntInside], inside);
}

// pool_words: the size of out_ops, which the host allocated from the total the count stage found
__global__ __launch_bounds__(256) void jst_proj_emit_kernel(const jst_project_params P, uint64_t pool_words)
{
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    const uint32_t n_slots = slot_count(P.counts, P.cap);
    bool bad = false, changed = false;
    if (s < n_slots) {
        const unsigned long long off = P.slot_off[s];
        const uint32_t nw = P.slot_words[s];
        bad = off + nw > pool_words;
        if (!bad) {
            jst_proj_write_sink S;
            S.out = P.out_ops + off;
            S.cap = nw;
            jst_proj_result R;
            spm_jst_aln a;
            bad = !jproj_run(P, s, S, R, a) || R.n_words != nw; // (both walks instantiate the same code)
            if (!bad) {
                changed = nw != a.cigar_len;
                for (uint32_t w = 0; !changed && w < nw; ++w)
                    changed = P.out_ops[off + w] != P.ops[a.cigar_off + w];
            }
        }
    }
    count_flagged(&P.counts[kProjCntBad], bad);
    count_flagged(&P.counts[kProjCntChanged], changed);
}

__global__ __launch_bounds__(256) void jst_proj_gather_kernel(const jst_project_params P)
{
    const unsigned long long i = blockIdx.x * 256ull + threadIdx.x;
    if (i >= P.n)
        return;
    const spm_jst_aln a = P.recs[i];
    spm_jst_ref_aln o;
    o.ref_begin = o.ref_end = 0;
    o.haplotype = a.haplotype;
    o.pattern = a.pattern;
    o.score = a.score;
    o.ref_score = 0;
    o.cigar_off = o.cigar_len = 0;
    if (a.cigar_off < P.n_ops) { // (the representatives stage has counted the records this does not hold for)
        const uint32_t s = P.sid[a.cigar_off];
        if (s < P.cap) {
            o.ref_begin = P.slot_range[2 * (uint64_t)s];
            o.ref_end = P.slot_range[2 * (uint64_t)s + 1];
            o.ref_score = P.slot_score[s];
            o.cigar_off = (uint32_t)P.slot_off[s];
            o.cigar_len = P.slot_words[s];
        }
    }
    P.out[i] = o;
}

} // namespace spm_hip

extern "C" void spm_hip_jst_ref_alns_destroy(spm_jst_ref_alns *a)
{
    if (!a)
        return;
    if (a->ctx && (a->d_recs || a->d_ops))
        hipStreamSynchronize(a->ctx->stream);
    hipFree(a->d_recs);
    hipFree(a->d_ops);
    delete a;
}

extern "C" int spm_hip_jst_alns_project(spm_jst_alns *a, uint32_t flags, spm_jst_ref_alns **out)
{
    using namespace spm_hip;
    if (!a || !out)
        return SPM_E_INVALID;
    spm_ctx *ctx = a->ctx;
    const auto t_call = clk::now();
    if (flags) {
        SPM_SET_ERR(ctx, "spm_hip_jst_alns_project: unknown flag bits 0x%x", flags);
        return SPM_E_INVALID;
    }
    if (a->begin_only) {
        SPM_SET_ERR(ctx, "spm_hip_jst_alns_project: these alignments were made with SPM_ALIGN_BEGIN_ONLY: there is no "
                         "transcript to project");
        return SPM_E_INVALID;
    }
    spm_jst *J = a->jst;
    const spm_patterns *ps = a->patterns;
    if (!J || !ps) {
        SPM_SET_ERR(ctx, "spm_hip_jst_alns_project: these alignments name no tree");
        return SPM_E_INVALID;
    }
    if (!J->indexed || J->generation != a->generation) {
        SPM_SET_ERR(ctx, "spm_hip_jst_alns_project: the tree has been indexed again since the search behind these alignments "
                         "(the tables the projection walks are gone); search and align again");
        return SPM_E_INVALID;
    }
    const uint64_t n = a->n, n_src_ops = a->n_ops;
    if (n > 0xFFFFFFFFull) {
        SPM_SET_ERR(ctx, "spm_hip_jst_alns_project: more than 2^32 - 1 records");
        return SPM_E_UNSUPPORTED;
    }
    SPM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    std::unique_ptr<spm_jst_ref_alns, void (*)(spm_jst_ref_alns *)> R(new spm_jst_ref_alns, spm_hip_jst_ref_alns_destroy);
    R->ctx = ctx;
    R->n = n;
    R->stats.n_alns = n;
    R->n_patterns = ps->n;
    R->n_ref = J->ref->n;
    R->jst = J;
    R->patterns = ps;
    hipStream_t st = ctx->stream;
    float ms_rep = 0, ms_count = 0, ms_emit = 0, ms_gather = 0;
    uint64_t n_slots = 0;
    if (n) {
        if (n_src_ops == 0 || !a->d_ops || !a->d_recs) {
            SPM_SET_ERR(ctx, "spm_hip_jst_alns_project: %llu records but no transcript pool", (unsigned long long)n);
            return SPM_E_INVALID;
        }
        SPM_TRY(spm_align_tables(ps)); // the needles' ranks on the device (built once per set)
        const uint32_t n32 = (uint32_t)n;
        const uint32_t cap = (uint32_t)std::min<uint64_t>(n, n_src_ops);
        hip_events<6> ev;
        SPM_HIP_CHECK(ctx, ev.create());
        size_t b_flag = 0, b_wide = 0;
        SPM_HIP_CHECK(ctx, slot_stage_tmp_bytes(ctx, n_src_ops, &b_flag));
        SPM_HIP_CHECK(ctx, exclusive_sum_tmp_bytes<unsigned long long>(ctx, counted<unsigned long long>(widen_op{nullptr}), cap,
                                                                       &b_wide));
        const size_t tmp_bytes = std::max(b_flag, b_wide);
        jst_project_params P{};
        unsigned long long *d_off = nullptr; // (P.slot_off, writable for the sum)
        uint8_t *d_tmp = nullptr;
        scratch_layout L;
        L.take(P.rep, n_src_ops);
        L.take(P.sid, n_src_ops);
        L.take(P.slot_rec, cap);
        L.take(P.slot_range, 2 * (size_t)cap);
        L.take(P.slot_words, cap);
        L.take(P.slot_score, cap);
        L.take(d_off, cap);
        L.take(P.counts, kProjCnts);
        L.take(d_tmp, tmp_bytes);
        SPM_TRY(ensure_scratch(ctx, L.bytes()));
        L.bind(ctx->d_scratch);
        SPM_HIP_CHECK(ctx, hipMalloc(&R->d_recs, n * sizeof(spm_jst_ref_aln)));

        P.J = J->dev();
        P.recs = a->d_recs;
        P.n = n32;
        P.ops = a->d_ops;
        P.ranks = ps->d_al_ranks;
        P.offsets = ps->d_al_offsets;
        P.m = ps->d_m;
        P.n_patterns = ps->n;
        P.n_ops = n_src_ops;
        P.cap = cap;
        P.slot_off = d_off;
        P.out_ops = nullptr;
        P.out = R->d_recs;
        // ---- representatives: one per distinct slot of the source pool, numbered in pool order ----
        SPM_HIP_CHECK(ctx, hipMemsetAsync(P.counts, 0, kProjCnts * 8, st));
        SPM_HIP_CHECK(ctx, hipEventRecord(ev[0], st));
        SPM_HIP_CHECK(ctx, slot_stage_enqueue(ctx, P.recs, n32, P.slots(), jproj_unusable{n_src_ops}, d_tmp, tmp_bytes));
        SPM_HIP_CHECK(ctx, hipEventRecord(ev[1], st));
        // ---- count: the projection of every slot with a counting sink, then where its words go ----
        SPM_HIP_CHECK(ctx, hipMemsetAsync(P.slot_words, 0, (size_t)cap * 4, st));
        SPM_HIP_CHECK(ctx, launch_1d(ctx, jst_proj_count_kernel, cap, P));
        SPM_HIP_CHECK(ctx, exclusive_sum(ctx, d_tmp, tmp_bytes, counted<unsigned long long>(widen_op{P.slot_words}), d_off, cap));
        SPM_HIP_CHECK(ctx, launch_1d<64>(ctx, slot_total_kernel, 1, P.counts, cap, P.slot_off, P.slot_words, kProjCntWords));
        SPM_HIP_CHECK(ctx, hipEventRecord(ev[2], st));
        // the one read-back that sizes the pool: {slots, errors, inside an insertion, -, words}
        SPM_HIP_CHECK(ctx, read_counts(ctx, P.counts, kProjCnts));
        unsigned long long *c = ctx->h_counters;
        n_slots = c[kProjCntSlots];
        const unsigned long long n_bad = c[kProjCntBad], total = c[kProjCntWords];
        R->stats.n_inside_insertion = c[kProjCntInside];
        if (n_bad || n_slots == 0 || n_slots > cap) {
            SPM_SET_ERR(ctx, "spm_hip_jst_alns_project: %llu records or transcript slots cannot be projected (a transcript "
                             "outside the pool, a begin outside its haplotype, or a transcript that does not consume its needle "
                             "and its haplotype stretch); nothing was projected", n_bad ? n_bad : (unsigned long long)n);
            return SPM_E_INVALID;
        }
        if (total > 0xFFFFFFFFull) { // decided before the emit launch
            SPM_SET_ERR(ctx, "spm_hip_jst_alns_project: the projected CIGAR pool would exceed 2^32 - 1 words");
            return SPM_E_UNSUPPORTED;
        }
        R->n_ops = total;
        SPM_HIP_CHECK(ctx, hipMalloc(&R->d_ops, std::max<uint64_t>(total, 1) * 4));
        P.out_ops = R->d_ops;
        // ---- emit, gather ----
        SPM_HIP_CHECK(ctx, hipEventRecord(ev[3], st));
        SPM_HIP_CHECK(ctx, launch_1d(ctx, jst_proj_emit_kernel, n_slots, P, total));
        SPM_HIP_CHECK(ctx, hipEventRecord(ev[4], st));
        SPM_HIP_CHECK(ctx, launch_1d(ctx, jst_proj_gather_kernel, n, P));
        SPM_HIP_CHECK(ctx, hipEventRecord(ev[5], st));
        // ---- the host view: record i of the source's host view through the slot tables ----
        slot_host_map slot(n_src_ops);
        std::vector<uint32_t> words(n_slots);
        std::vector<int32_t> score(n_slots);
        std::vector<unsigned long long> range(2 * n_slots), woff(n_slots);
        R->host_ops.resize(total);
        SPM_HIP_CHECK(ctx, hipMemcpyAsync(c, P.counts, kProjCnts * 8, hipMemcpyDeviceToHost, st));
        SPM_HIP_CHECK(ctx, slot.download(ctx, P.slots()));
        SPM_HIP_CHECK(ctx, hipMemcpyAsync(words.data(), P.slot_words, n_slots * 4, hipMemcpyDeviceToHost, st));
        SPM_HIP_CHECK(ctx, hipMemcpyAsync(score.data(), P.slot_score, n_slots * 4, hipMemcpyDeviceToHost, st));
        SPM_HIP_CHECK(ctx, hipMemcpyAsync(range.data(), P.slot_range, n_slots * 16, hipMemcpyDeviceToHost, st));
        SPM_HIP_CHECK(ctx, hipMemcpyAsync(woff.data(), d_off, n_slots * 8, hipMemcpyDeviceToHost, st));
        if (total)
            SPM_HIP_CHECK(ctx, hipMemcpyAsync(R->host_ops.data(), R->d_ops, total * 4, hipMemcpyDeviceToHost, st));
        SPM_HIP_CHECK(ctx, hipStreamSynchronize(st));
        hipEventElapsedTime(&ms_rep, ev[0], ev[1]);
        hipEventElapsedTime(&ms_count, ev[1], ev[2]);
        hipEventElapsedTime(&ms_emit, ev[3], ev[4]);
        hipEventElapsedTime(&ms_gather, ev[4], ev[5]);
        if (c[kProjCntBad]) {
            SPM_SET_ERR(ctx, "spm_hip_jst_alns_project: %llu transcript slots came out of the emit stage differently from the "
                             "count stage", c[kProjCntBad]);
            return SPM_E_INVALID;
        }
        R->stats.n_changed = c[kProjCntChanged];
        if (a->host.size() != n) {
            SPM_SET_ERR(ctx, "spm_hip_jst_alns_project: the source holds no host view");
            return SPM_E_INVALID;
        }
        R->host.resize(n);
        for (uint64_t i = 0; i < n; ++i) {
            const spm_jst_aln &x = a->host[i];
            const uint32_t s = slot.of(x.cigar_off);
            if (s >= n_slots) {
                SPM_SET_ERR(ctx, "spm_hip_jst_alns_project: host record %llu names no projected slot", (unsigned long long)i);
                return SPM_E_INVALID;
            }
            R->host[i] = spm_jst_ref_aln{range[2 * (uint64_t)s], range[2 * (uint64_t)s + 1], x.haplotype, x.pattern, x.score,
                                         score[s], (uint32_t)woff[s], words[s]};
        }
    }
    R->stats.ms_representatives = ms_rep;
    R->stats.ms_count = ms_count;
    R->stats.ms_emit = ms_emit;
    R->stats.ms_gather = ms_gather;
    R->stats.ms_total = ms_rep + ms_count + ms_emit + ms_gather;
    R->stats.n_projected = n_slots;
    R->stats.n_ops = R->n_ops;
    R->stats.ms_host = ms_since(t_call);
    if (spm_trace_on())
        fprintf(stderr, "[spm_hip] jst project: %llu records, %llu slots -> %llu words (%llu changed, %llu inside an insertion): "
                        "representatives %.3f ms, count %.3f, emit %.3f, gather %.3f; %.3f ms in all\n", (unsigned long long)n,
                (unsigned long long)n_slots, (unsigned long long)R->n_ops, (unsigned long long)R->stats.n_changed,
                (unsigned long long)R->stats.n_inside_insertion, ms_rep, ms_count, ms_emit, ms_gather, R->stats.ms_host);
    *out = R.release();
    return SPM_OK;
}

extern "C" int spm_hip_jst_ref_alns_view(spm_jst_ref_alns *a, const spm_jst_ref_aln **records, uint64_t *n, const uint32_t **ops,
                                         uint64_t *n_ops)
{
    if (!a)
        return SPM_E_INVALID;
    return pool_out(pool_src<spm_jst_ref_aln>{a->host.data(), a->n, a->host_ops.data(), a->n_ops}, records, n, ops, n_ops);
}

extern "C" int spm_hip_jst_ref_alns_device(spm_jst_ref_alns *a, const void **records, uint64_t *n, const void **ops,
                                           uint64_t *n_ops)
{
    if (!a)
        return SPM_E_INVALID;
    return pool_out(pool_src<void, void, void>{a->d_recs, a->n, a->d_ops, a->n_ops}, records, n, ops, n_ops);
}

extern "C" int spm_hip_jst_ref_alns_stats(const spm_jst_ref_alns *a, spm_jst_project_stats *out)
{
    if (!a || !out)
        return SPM_E_INVALID;
    *out = a->stats;
    return SPM_OK;
}

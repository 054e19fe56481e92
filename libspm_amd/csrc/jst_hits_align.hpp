// jst_hits_align.hpp -- begins and alignments of the hits of a pan-genome search (spm_hip_jst_hits_align; contract in
// spm_hip.h, scheme in DESIGN.md 4.6), the result object spm_jst_alns, and what the call shares with
// spm_hip_jst_selection_align (jst_locate.hpp): jst_align_segments (distinct segment hits -> their alignments on the device)
// and jst_alns_download / jst_alns_close (host view, statistics).  gfx950.  Unit: jst_align.hip.  The fan-out of the
// alignments, jst_aln_fanout_kernel, is here, over the walker of jst_fanout.hpp.
#pragma once

#include "internal.hpp"
#include "jst_fanout.hpp"
#include "jst_handles.hpp"

namespace spm_hip
{

struct jst_alnfan_params
{
    const spm_aln *segs; // one alignment per segment hit, context-buffer coordinates (stage A / stage B of align.hpp)
    uint64_t n_segs;
    jst_ctx_tables T;
    spm_jst_aln *out;
    unsigned long long *out_count;
    uint64_t out_cap;
};

// The alignment fan-out: one thread per segment alignment.  It is dropped if its last symbol lies in the left context; else
// every haplotype of the context's group gets a record with its own coordinates and the SHARED transcript (cigar_off /
// cigar_len of the segment alignment).
__global__ __launch_bounds__(256) void jst_aln_fanout_kernel(jst_dev J, jst_alnfan_params F)
{
    jst_fan_out<spm_aln>(
        J, F.T, F.n_segs, F.out_count, F.out_cap,
        [&](uint64_t t, spm_aln &al, jst_fan_item &it) {
            al = F.segs[t];
            it.probe = it.last = al.end - 1; // the alignment's last symbol: a symbol of its own context
            it.at = al.end;
            it.span = al.end - al.begin;
            return al.end > 0 && al.begin <= al.end;
        },
        [&](const spm_aln &al, unsigned long long slot, uint32_t h, uint64_t ctx_lo, uint64_t local_end) {
            spm_jst_aln o;
            o.end = ctx_lo + local_end;
            o.begin = o.end - (al.end - al.begin);
            o.haplotype = h;
            o.pattern = al.pattern;
            o.score = al.score;
            o.cigar_off = al.cigar_off;
            o.cigar_len = al.cigar_len;
            o.reserved = 0;
            F.out[slot] = o;
        });
}

} // namespace spm_hip

extern "C" void spm_hip_jst_alns_destroy(spm_jst_alns *a)
{
    if (!a)
        return;
    if (a->ctx && (a->d_recs || a->d_ops))
        hipStreamSynchronize(a->ctx->stream);
    hipFree(a->d_recs);
    hipFree(a->d_ops);
    delete a;
}

// exact sets: nothing to compute -- begin = pos, end = pos + |P|, transcript |P|=, filled on the host
static int jst_fill_exact_alns(spm_ctx *ctx, const spm_patterns *ps, const std::vector<spm_hit> &kh,
                               const std::vector<uint32_t> &cig_off, bool begin_only, spm_aln *d_seg_alns, spm_jst_alns *A)
{
    const uint64_t nk = kh.size();
    std::vector<spm_aln> sa(nk);
    for (uint64_t i = 0; i < nk; ++i) {
        const uint32_t m = (uint32_t)ps->m[kh[i].pattern];
        sa[i] = spm_aln{kh[i].pos, kh[i].pos + m, kh[i].pattern, kh[i].score, begin_only ? 0u : cig_off[i], begin_only ? 0u : 1u};
        if (!begin_only)
            A->host_ops[cig_off[i]] = (m << 4) | SPM_CIGAR_EQ;
    }
    SPM_HIP_CHECK(ctx, hipMemcpyAsync(d_seg_alns, sa.data(), nk * sizeof(spm_aln), hipMemcpyHostToDevice, ctx->stream));
    if (A->n_ops)
        SPM_HIP_CHECK(ctx, hipMemcpyAsync(A->d_ops, A->host_ops.data(), A->n_ops * 4, hipMemcpyHostToDevice, ctx->stream));
    SPM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream)); // (sa is read by the copy)
    return SPM_OK;
}

// the order of spm_hip_jst_hits_view: (haplotype, pos, pattern, score), pos = end (Myers) / begin (exact)
static void jst_sort_alns_host(std::vector<spm_jst_aln> &v, bool myers)
{
    std::sort(v.begin(), v.end(), [myers](const spm_jst_aln &a, const spm_jst_aln &b) {
        if (a.haplotype != b.haplotype)
            return a.haplotype < b.haplotype;
        const uint64_t pa = myers ? a.end : a.begin, pb = myers ? b.end : b.begin;
        if (pa != pb)
            return pa < pb;
        if (a.pattern != b.pattern)
            return a.pattern < b.pattern;
        return a.score < b.score;
    });
}

// What the two pan-genome align calls share.  From the distinct segment hits kh (pool order) and lo[i], the start of hit i's
// context, to their alignments on the device (*d_seg_alns, owned by `tmp`) and the transcript pool in A: sizes the pool,
// ends the caller's work-list clock (ms_worklist = time since t_list), allocates, runs stage A / stage B or the exact fill.
static int jst_align_segments(spm_ctx *ctx, spm_jst *J, const spm_patterns *ps, const std::vector<spm_hit> &kh,
                              const std::vector<uint64_t> &lo, bool begin_only, clk::time_point t_list, const char *who,
                              dev_scratch &tmp, spm_jst_alns *A, spm_aln **d_seg_alns)
{
    using namespace spm_hip;
    const bool myers = ps->is_myers();
    const uint64_t nk = kh.size();
    std::vector<uint32_t> cig_off(nk, 0);
    uint64_t total_ops = 0;
    for (uint64_t i = 0; i < nk; ++i) {
        cig_off[i] = (uint32_t)total_ops;
        total_ops += myers ? 2 * (uint64_t)std::max(0, kh[i].score) + 1 : 1;
    }
    if (total_ops > 0xFFFFFFFFull) { // (every hit has a word: this bounds the number of hits too)
        SPM_SET_ERR(ctx, "%s: the CIGAR pool would exceed 2^32 words", who);
        return SPM_E_UNSUPPORTED;
    }
    A->n_ops = begin_only ? 0 : total_ops;
    A->host_ops.resize(A->n_ops);
    A->stats.ms_worklist = ms_since(t_list);
    SPM_HIP_CHECK(ctx, tmp.alloc(d_seg_alns, nk * sizeof(spm_aln)));
    if (A->n_ops)
        SPM_HIP_CHECK(ctx, hipMalloc(&A->d_ops, A->n_ops * 4));
    if (!myers)
        return jst_fill_exact_alns(ctx, ps, kh, cig_off, begin_only, *d_seg_alns, A);
    align_work W{}; // over the context buffer: lo = the start of the hit's context, positions as they are (pos_offset 0)
    W.ps = ps;
    W.text = J->ctx_text;
    W.hits = kh.data();
    W.n = nk;
    W.lo = lo.data();
    W.cig_off = cig_off.data();
    W.begin_only = begin_only;
    W.d_recs = *d_seg_alns;
    W.d_ops = A->d_ops;
    W.n_ops = A->n_ops;
    W.h_ops = A->host_ops.data();
    W.who = who;
    spm_align_stats as{};
    SPM_TRY(align_run(ctx, W, as));
    A->stats.ms_begin = as.ms_begin;
    A->stats.ms_cigar = as.ms_cigar;
    A->stats.begin_lane = as.begin_lane;
    A->stats.begin_wave = as.begin_wave;
    A->stats.cigar_lane = as.cigar_lane;
    A->stats.cigar_wave = as.cigar_wave;
    A->stats.cigar_wave_global = as.cigar_wave_global;
    return SPM_OK;
}

// ... and their tail in two steps.  The host view of A->d_recs, once the caller's last stage is enqueued; behind its
// synchronisation every event of the call has happened, and the caller reads its own stage's time into ms_fanout.
static int jst_alns_download(spm_ctx *ctx, spm_jst_alns *A)
{
    A->host.resize(A->n);
    SPM_HIP_CHECK(ctx, hipMemcpyAsync(A->host.data(), A->d_recs, A->n * sizeof(spm_jst_aln), hipMemcpyDeviceToHost,
                                      ctx->stream));
    SPM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return SPM_OK;
}
// ... then the order of spm_hip_jst_hits_view and the statistics; returns the host sort's ms (work list time to one caller)
static float jst_alns_close(spm_jst_alns *A, uint64_t nk, bool myers, clk::time_point t_call)
{
    const auto t_sort = clk::now();
    jst_sort_alns_host(A->host, myers);
    const float ms_sort = ms_since(t_sort);
    A->stats.ms_total = A->stats.ms_begin + A->stats.ms_cigar + A->stats.ms_fanout;
    A->stats.n_alns = A->n;
    A->stats.n_segment_alns = nk;
    A->stats.n_ops = A->n_ops;
    A->stats.ms_host = ms_since(t_call);
    return ms_sort;
}

extern "C" int spm_hip_jst_hits_align(spm_jst_hits *h, uint32_t flags, spm_jst_alns **out)
{
    using namespace spm_hip;
    if (!h || !out || (flags & ~SPM_ALIGN_BEGIN_ONLY))
        return SPM_E_INVALID;
    spm_ctx *ctx = h->ctx;
    const auto t_call = clk::now();
    if (h->selected) {
        SPM_SET_ERR(ctx, "spm_hip_jst_hits_align: these hits are a selection, which keeps no map from its records back to the "
                         "search's segment hits; align the search's own result, or the selection's records with "
                         "spm_hip_jst_selection_align");
        return SPM_E_INVALID;
    }
    if (!h->alignable) {
        SPM_SET_ERR(ctx, "spm_hip_jst_hits_align: these hits do not keep their segment hits; search with "
                         "spm_scan_opts.flags & SPM_SCAN_ALIGNABLE");
        return SPM_E_INVALID;
    }
    spm_jst *J = h->jst;
    const spm_patterns *ps = h->patterns;
    if (!J->indexed || J->generation != h->generation) {
        SPM_SET_ERR(ctx, "spm_hip_jst_hits_align: the tree has been indexed again since this search (its context buffer is "
                         "gone); search again");
        return SPM_E_INVALID;
    }
    SPM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    std::unique_ptr<spm_jst_alns, void (*)(spm_jst_alns *)> A(new spm_jst_alns, spm_hip_jst_alns_destroy);
    A->ctx = ctx;
    A->n = h->n;
    const bool begin_only = (flags & SPM_ALIGN_BEGIN_ONLY) != 0;
    A->jst = J;
    A->patterns = ps;
    A->generation = J->generation;
    A->begin_only = begin_only;
    const bool myers = ps->is_myers();
    const uint64_t n = h->n;
    hipStream_t st = ctx->stream;

    // ---- the segment hits that end on an owned symbol, in the order (pattern, position in the context buffer) ----
    struct kept_hit
    {
        spm_hit hit;
        uint64_t lo;
    };
    std::vector<kept_hit> kept;
    if (n && h->seg) {
        const void *d_seg = nullptr;
        uint64_t n_seg = 0;
        int rc = spm_hip_hits_device(h->seg, &d_seg, &n_seg);
        if (rc != SPM_OK)
            return rc;
        std::vector<spm_hit> sh(n_seg);
        SPM_TRY(J->fetch_ctx_tables()); // once per index generation
        if (n_seg)
            SPM_HIP_CHECK(ctx, hipMemcpyAsync(sh.data(), d_seg, n_seg * sizeof(spm_hit), hipMemcpyDeviceToHost, st));
        SPM_HIP_CHECK(ctx, hipStreamSynchronize(st));
        J->h_generation = J->generation;
        const std::vector<uint64_t> &off = J->h_ctx_off;
        kept.reserve(n_seg);
        for (uint64_t i = 0; i < n_seg; ++i) {
            const spm_hit &x = sh[i];
            if (x.pattern >= ps->n) {
                SPM_SET_ERR(ctx, "spm_hip_jst_hits_align: segment hit of pattern %u outside the set", x.pattern);
                return SPM_E_INVALID;
            }
            const uint64_t last = myers ? x.pos - 1 : x.pos + (uint64_t)ps->m[x.pattern] - 1; // (pos = 0 wraps: rejected below)
            if (last >= J->ctx_bytes || J->n_ctx == 0) {
                SPM_SET_ERR(ctx, "spm_hip_jst_hits_align: segment hit %llu lies outside the context buffer", (unsigned long long)i);
                return SPM_E_INVALID;
            }
            const uint64_t c = (uint64_t)(std::upper_bound(off.begin(), off.begin() + (long)J->n_ctx, last) - off.begin()) - 1;
            if (last - off[c] < J->h_ctx_owned[c])
                continue; // ends in the left context: the previous block's context reports it
            kept.push_back({x, off[c]});
        }
        std::sort(kept.begin(), kept.end(), [](const kept_hit &a, const kept_hit &b) {
            if (a.hit.pattern != b.hit.pattern)
                return a.hit.pattern < b.hit.pattern;
            if (a.hit.pos != b.hit.pos)
                return a.hit.pos < b.hit.pos;
            return a.hit.score < b.hit.score;
        });
    }
    const uint64_t nk = kept.size();
    std::vector<spm_hit> kh(nk);
    std::vector<uint64_t> lo(nk);
    for (uint64_t i = 0; i < nk; ++i) {
        kh[i] = kept[i].hit;
        lo[i] = kept[i].lo;
    }
    if (nk) {
        dev_scratch tmp; // (released inside this block: its hipFree is part of ms_host, as it always was)
        spm_aln *d_seg_alns = nullptr;
        unsigned long long *d_count = nullptr;
        SPM_HIP_CHECK(ctx, tmp.alloc(&d_count, 8));
        SPM_HIP_CHECK(ctx, hipMalloc(&A->d_recs, n * sizeof(spm_jst_aln)));
        SPM_TRY(jst_align_segments(ctx, J, ps, kh, lo, begin_only, t_call, "spm_hip_jst_hits_align", tmp, A.get(), &d_seg_alns));
        // ---- the fan-out: one record per (haplotype, hit), the transcript shared ----
        hip_events<2> ev;
        SPM_HIP_CHECK(ctx, ev.create());
        const jst_alnfan_params F{d_seg_alns, nk, J->ctx_tables(), A->d_recs, d_count, n};
        SPM_HIP_CHECK(ctx, hipMemsetAsync(d_count, 0, 8, st));
        SPM_HIP_CHECK(ctx, hipEventRecord(ev[0], st));
        hipLaunchKernelGGL(jst_aln_fanout_kernel, dim3((unsigned)std::min<uint64_t>((nk + 255) / 256, (uint64_t)ctx->n_cu * 64)),
                           dim3(256), 0, st, J->dev(), F);
        SPM_HIP_CHECK(ctx, hipGetLastError());
        SPM_HIP_CHECK(ctx, hipEventRecord(ev[1], st));
        unsigned long long n_out = 0;
        SPM_HIP_CHECK(ctx, hipMemcpyAsync(&n_out, d_count, 8, hipMemcpyDeviceToHost, st));
        SPM_HIP_CHECK(ctx, hipStreamSynchronize(st));
        hipEventElapsedTime(&A->stats.ms_fanout, ev[0], ev[1]);
        if (n_out != n) {
            SPM_SET_ERR(ctx, "spm_hip_jst_hits_align: the fan-out wrote %llu alignment records for %llu hits", n_out,
                        (unsigned long long)n);
            return SPM_E_INVALID;
        }
        SPM_TRY(jst_alns_download(ctx, A.get()));
    } else if (n) {
        SPM_SET_ERR(ctx, "spm_hip_jst_hits_align: %llu hits but no segment hit to align", (unsigned long long)n);
        return SPM_E_INVALID;
    } else
        A->stats.ms_worklist = ms_since(t_call); // (nothing to align: an empty pool)
    jst_alns_close(A.get(), nk, myers, t_call);
    if (spm_trace_on())
        fprintf(stderr, "[spm_hip] jst align: %llu segment alignments -> %llu records%s: begins %.3f ms, transcripts %.3f, "
                        "fan-out %.3f; %.3f ms in all (work list %.3f)\n", (unsigned long long)nk, (unsigned long long)n,
                begin_only ? " (begins only)" : "", A->stats.ms_begin, A->stats.ms_cigar, A->stats.ms_fanout,
                A->stats.ms_host, A->stats.ms_worklist);
    *out = A.release();
    return SPM_OK;
}

extern "C" int spm_hip_jst_alns_view(spm_jst_alns *a, const spm_jst_aln **records, uint64_t *n, const uint32_t **ops,
                                     uint64_t *n_ops)
{
    if (!a)
        return SPM_E_INVALID;
    return pool_out(pool_src<spm_jst_aln>{a->host.data(), a->n, a->host_ops.data(), a->n_ops}, records, n, ops, n_ops);
}

extern "C" int spm_hip_jst_alns_device(spm_jst_alns *a, const void **records, uint64_t *n, const void **ops, uint64_t *n_ops)
{
    if (!a)
        return SPM_E_INVALID;
    return pool_out(pool_src<void, void, void>{a->d_recs, a->n, a->d_ops, a->n_ops}, records, n, ops, n_ops);
}

extern "C" int spm_hip_jst_alns_stats(const spm_jst_alns *a, spm_jst_align_stats *out)
{
    if (!a || !out)
        return SPM_E_INVALID;
    *out = a->stats;
    return SPM_OK;
}

// jst_locate.hpp -- begins and alignments of the records a pan-genome SELECTION kept (spm_hip_jst_selection_align; contract
// in spm_hip.h, scheme in DESIGN.md 4.6).  gfx950.  Unit: jst_align.hip, with jst_hits_align.hpp, whose host helpers it calls.
//
// jst_fanout_kernel is a bijection from (segment hit ending on an owned symbol, member haplotype of its context) to
// haplotype record.  A selection keeps records, not segment hits, so the map is inverted per kept record from the tables of
// the index, which are resident anyway:
//   record (h, pattern, pos, score), last symbol l = pos - 1 (Myers) / pos + |P| - 1 (exact)
//   block j of haplotype h that owns l:  hap_start[j][h] <= l < hap_start[j + 1][h]   (binary search down column h)
//   context c = ctx_base[cell(j, h)] + (local_id[j][h] & 0x7FFF)
//   ctx_lo(h) = hap_start[j][h] - min(window - 1, hap_start[j][h])
//   segment hit (pattern, ctx_off[c] + pos - ctx_lo(h), score) in the context buffer.
// Records of haplotypes that share a context land on the same segment hit: the DISTINCT ones are aligned once by the kernels
// of align.hpp, then gathered, which preserves the sharing of the tree.
//   jst_locate_kernel       one lane per kept record: the inversion, key = pattern << ctx_bits | context position
//   (hipcub radix sort of (key, arrival index) over the key's bits)
//   jst_locate_heads_kernel head flag of every run of equal keys; the scores of a run must agree
//   (hipcub exclusive sum of the head flags: the number u of every distinct segment hit)
//   jst_locate_emit_kernel  heads write the compact spm_hit list (already in pool order), every record uid[arrival] = u
//   jst_aln_gather_kernel   one lane per kept record i: record i + seg_alns[uid[i]] -> the 40-byte spm_jst_aln i
// Between emit and gather: jst_align_segments; the end: jst_alns_download / _close (jst_hits_align.hpp's, shared with spm_hip_jst_hits_align).
// The scratch is laid out with scratch_layout.hpp; the launches, the sort, the sum and the events are device_order.hpp's; the
// count of the flagged lanes is wave.hpp's.
#pragma once

#include "internal.hpp"
#include "device_order.hpp"
#include "jst_handles.hpp"
#include "jst_hits_align.hpp"
#include "scratch_layout.hpp"
#include "select_plan.hpp"
#include "wave.hpp"

namespace spm_hip
{

struct jst_locate_params
{
    const unsigned long long *recs; // the selection's records as 8-byte words, three each: pos | pattern << 32 + haplotype |
                                    // reserved << 32 + score
    uint32_t n;
    // the index (all of it bounds-checked against the sizes below before it is read)
    const uint64_t *hap_start; // [(n_blocks + 1) * n_hap]
    jst_ctx_tables T;          // (ctx_block is not read: the cell follows from the block and the haplotype)
    uint64_t jb, je;
    uint32_t n_hap, n_groups, window;
    const int32_t *m;          // needle lengths [n_patterns]
    uint32_t n_patterns;
    uint32_t report_begin;     // exact sets: pos is the begin, the last symbol pos + |P| - 1
    uint32_t ctx_bits;         // bits of a context position (<= ctx_bytes)
    // out
    unsigned long long *keys;  // [n] arrival order
    uint32_t *idx;             // [n]
    int32_t *score;            // [n]
    unsigned long long *counts; // [0] distinct segment hits (emit), [1] records that cannot be located / disagree
};

// One lane per kept record.  The records are read as jst_select_keys_kernel reads them: 768 contiguous 8-byte words per
// workgroup, handed to their lanes through LDS.  The selection's device order is haplotype-major, so the lanes of a wave
// walk the same column of hap_start.  Every table index is tested against the table's size first: whatever a record holds,
// the kernel reads inside the tables or counts an error.
__global__ __launch_bounds__(256) void jst_locate_kernel(const jst_locate_params P)
{
    __shared__ unsigned long long s_w[3 * 256];
    const unsigned long long base = (unsigned long long)blockIdx.x * 256ull;
    const unsigned long long n_words = 3ull * P.n;
#pragma unroll
    for (uint32_t r = 0; r < 3; ++r) {
        const unsigned long long w = base * 3ull + r * 256u + threadIdx.x;
        if (w < n_words)
            s_w[r * 256u + threadIdx.x] = P.recs[w];
    }
    __syncthreads();
    const unsigned long long i = base + threadIdx.x;
    const bool valid = i < P.n;
    bool ok = false;
    unsigned long long key = ~0ull;
    int32_t sc = 0;
    if (valid) {
        const unsigned long long pos = s_w[3 * threadIdx.x], w_hp = s_w[3 * threadIdx.x + 1];
        const uint32_t h = (uint32_t)w_hp, pat = (uint32_t)(w_hp >> 32);
        sc = (int32_t)(uint32_t)s_w[3 * threadIdx.x + 2];
        ok = h < P.n_hap && pat < P.n_patterns && P.jb < P.je;
        uint64_t last = 0;
        if (ok) {
            const uint64_t len = P.report_begin ? (uint64_t)max(P.m[pat], 0) : 0ull;
            last = pos + len - 1;                     // exact: pos + |P| - 1; Myers: pos - 1
            ok = pos + len >= 1 && pos + len >= pos;  // (pos = 0 of a Myers hit, or a wrap: no last symbol)
        }
        uint64_t j = P.jb;
        if (ok) {
            // the largest j in [jb, je] with hap_start[j][h] <= last (the column is non-decreasing; among equal starts the
            // last one is the block that owns something)
            uint64_t lo = P.jb, hi = P.je + 1; // hap_start[lo] <= last < hap_start[hi], once the first test holds
            ok = P.hap_start[lo * P.n_hap + h] <= last;
            while (ok && hi - lo > 1) {
                const uint64_t mid = (lo + hi) >> 1;
                if (P.hap_start[mid * P.n_hap + h] <= last)
                    lo = mid;
                else
                    hi = mid;
            }
            j = lo;
            ok = ok && j < P.je; // (j == je: beyond the indexed blocks)
        }
        if (ok) {
            const uint64_t jr = j - P.jb;
            const uint16_t v = P.T.local_id[jr * P.n_hap + h];
            const uint64_t cb = jr * P.n_groups + h / kJstGroup;
            ok = v != kJstNone;
            if (ok) {
                const uint64_t c = P.T.ctx_base[cb] + (uint64_t)(v & 0x7FFFu);
                ok = c < P.T.ctx_base[cb + 1] && c < P.T.n_ctx;
                if (ok) {
                    const uint64_t a = P.hap_start[j * P.n_hap + h];
                    const uint64_t ctx_lo = a - min((uint64_t)(P.window ? P.window - 1 : 0), a);
                    const uint64_t off = P.T.ctx_off[c], len_c = P.T.ctx_off[c + 1] - off;
                    // the last symbol inside the context and not in its left context; the reported position inside it
                    ok = pos >= ctx_lo && last >= ctx_lo && last - ctx_lo < len_c && last - ctx_lo >= P.T.ctx_owned[c];
                    const uint64_t at = off + (pos - ctx_lo);
                    ok = ok && (P.ctx_bits >= 64 || (at >> P.ctx_bits) == 0);
                    if (ok)
                        key = (P.ctx_bits < 64 ? (unsigned long long)pat << P.ctx_bits : 0ull) | at;
                }
            }
        }
        P.keys[i] = key; // (an unlocated record sorts last; the call fails before anything reads it)
        P.idx[i] = (uint32_t)i;
        P.score[i] = sc;
    }
    count_flagged(&P.counts[1], valid && !ok);
}

// One lane per sorted record: 1 where a run of equal keys begins.  Records of one run name the same segment hit, so their
// scores agree; a run that disagrees is counted as an error (one atomic per wave).
__global__ __launch_bounds__(256) void jst_locate_heads_kernel(const unsigned long long *__restrict__ keys,
                                                                 const uint32_t *__restrict__ idx,
                                                                 const int32_t *__restrict__ score, uint32_t n,
                                                                 uint8_t *__restrict__ head, unsigned long long *counts)
{
    const unsigned long long i = blockIdx.x * 256ull + threadIdx.x;
    bool bad = false;
    if (i < n) {
        const bool first = i == 0 || keys[i] != keys[i - 1];
        head[i] = first ? 1 : 0;
        bad = !first && score[idx[i]] != score[idx[i - 1]];
    }
    count_flagged(&counts[1], bad);
}

struct jloc_head_op
{
    const uint8_t *head;
    __device__ __forceinline__ uint32_t operator()(uint32_t i) const { return head[i]; }
};

// offs: exclusive sum of the head flags.  The heads write the distinct segment hits, which the sort has put in pool order
// (pattern, position in the context buffer); every record learns the number of its segment hit; the last lane writes the
// count the host reads back.
__global__ __launch_bounds__(256) void jst_locate_emit_kernel(const unsigned long long *__restrict__ keys,
                                                                const uint32_t *__restrict__ idx,
                                                                const int32_t *__restrict__ score,
                                                                const uint8_t *__restrict__ head,
                                                                const uint32_t *__restrict__ offs, uint32_t n, uint32_t ctx_bits,
                                                                spm_hit *__restrict__ list, uint32_t *__restrict__ uid,
                                                                unsigned long long *counts)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n)
        return;
    const uint32_t hd = head[i];
    const uint32_t u = offs[i] + hd - 1u; // (offs[0] = 0 and head[0] = 1: never wraps)
    const uint32_t from = idx[i];
    if (hd) {
        const unsigned long long key = keys[i];
        spm_hit o;
        o.pos = ctx_bits < 64 ? key & ((1ull << ctx_bits) - 1) : key;
        o.pattern = ctx_bits < 64 ? (uint32_t)(key >> ctx_bits) : 0u;
        o.score = score[from];
        list[u] = o;
    }
    uid[from] = u;
    if (i == n - 1)
        counts[0] = (unsigned long long)u + 1ull;
}

// One lane per kept record i: its own record (through LDS, as above) and the alignment of its segment hit give the
// spm_jst_aln i -- the haplotype's coordinates, the SHARED transcript.  The output index is the input index: no atomics, no
// slot reservation.  A record is five 8-byte words; the 1280 words of a workgroup leave through LDS, contiguous per wave.
__global__ __launch_bounds__(256) void jst_aln_gather_kernel(const unsigned long long *__restrict__ recs,
                                                               const uint32_t *__restrict__ uid,
                                                               const spm_aln *__restrict__ segs, uint32_t n, uint32_t n_segs,
                                                               uint32_t report_begin, unsigned long long *__restrict__ out)
{
    __shared__ unsigned long long s_w[5 * 256];
    const unsigned long long base = (unsigned long long)blockIdx.x * 256ull;
    const unsigned long long n_in = 3ull * n, n_out = 5ull * n;
#pragma unroll
    for (uint32_t r = 0; r < 3; ++r) {
        const unsigned long long w = base * 3ull + r * 256u + threadIdx.x;
        if (w < n_in)
            s_w[r * 256u + threadIdx.x] = recs[w];
    }
    __syncthreads();
    const unsigned long long i = base + threadIdx.x;
    unsigned long long o[5] = {0, 0, 0, 0, 0};
    if (i < n) {
        const unsigned long long pos = s_w[3 * threadIdx.x], w_hp = s_w[3 * threadIdx.x + 1];
        const uint32_t u = uid[i];
        if (u < n_segs) {
            const spm_aln a = segs[u];
            const unsigned long long span = a.end - a.begin;
            const unsigned long long end = report_begin ? pos + span : pos;
            o[0] = end - span;                                                              // begin
            o[1] = end;                                                                     // end
            o[2] = w_hp;                                                                    // haplotype | pattern << 32
            o[3] = (unsigned long long)(uint32_t)a.score | (unsigned long long)a.cigar_off << 32;
            o[4] = (unsigned long long)a.cigar_len;                                         // cigar_len | reserved << 32
        }
    }
    __syncthreads(); // every lane has read its record: the words may be overwritten
#pragma unroll
    for (uint32_t r = 0; r < 5; ++r)
        s_w[5 * threadIdx.x + r] = o[r];
    __syncthreads();
#pragma unroll
    for (uint32_t r = 0; r < 5; ++r) {
        const unsigned long long w = base * 5ull + r * 256u + threadIdx.x;
        if (w < n_out)
            out[w] = s_w[r * 256u + threadIdx.x];
    }
}

} // namespace spm_hip

static_assert(sizeof(spm_jst_aln) == 5 * 8 && sizeof(spm_jst_hit) == 3 * 8 && sizeof(spm_aln) == 32, "word layouts of the gather");

extern "C" int spm_hip_jst_selection_align(spm_jst_hits *h, uint32_t flags, spm_jst_alns **out)
{
    using namespace spm_hip;
    if (!h || !out)
        return SPM_E_INVALID;
    spm_ctx *ctx = h->ctx;
    if (flags & ~SPM_ALIGN_BEGIN_ONLY) {
        SPM_SET_ERR(ctx, "spm_hip_jst_selection_align: unknown flag bits 0x%x", flags & ~SPM_ALIGN_BEGIN_ONLY);
        return SPM_E_INVALID;
    }
    const auto t_call = clk::now();
    if (!h->selected) {
        SPM_SET_ERR(ctx, "spm_hip_jst_selection_align: these hits are a search's own result, not a selection; align them with "
                         "spm_hip_jst_hits_align, or select them first (a selection without flags is a sorted copy)");
        return SPM_E_INVALID;
    }
    if (!h->jst || !h->patterns) {
        SPM_SET_ERR(ctx, "spm_hip_jst_selection_align: this selection was made from a raw record buffer "
                         "(spm_hip_jst_records_select): it names no tree, and its records may stem from several block shards");
        return SPM_E_INVALID;
    }
    spm_jst *J = h->jst;
    const spm_patterns *ps = h->patterns;
    if (!J->indexed || J->generation != h->generation) {
        SPM_SET_ERR(ctx, "spm_hip_jst_selection_align: the tree has been indexed again since this search (its context buffer is "
                         "gone); search and select again");
        return SPM_E_INVALID;
    }
    const bool begin_only = (flags & SPM_ALIGN_BEGIN_ONLY) != 0;
    const bool myers = ps->is_myers();
    const uint64_t n = h->n;
    const jst_locate_plan plan = plan_jst_locate(n, ps->n, J->ctx_bytes); // decided before any launch
    if (plan.status != SPM_OK) {
        SPM_SET_ERR(ctx, "spm_hip_jst_selection_align: %s (%u + %u bits)", plan.why, plan.pat_bits, plan.ctx_bits);
        return plan.status;
    }
    SPM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    std::unique_ptr<spm_jst_alns, void (*)(spm_jst_alns *)> A(new spm_jst_alns, spm_hip_jst_alns_destroy);
    A->ctx = ctx;
    A->n = n;
    A->jst = J;
    A->patterns = ps;
    A->generation = J->generation;
    A->begin_only = begin_only;
    hipStream_t st = ctx->stream;
    uint64_t nk = 0;
    float ms_locate = 0, ms_gather = 0;
    if (n) {
        const uint32_t n32 = (uint32_t)n;
        hip_events<4> ev; // locate + order [0, 1], gather [2, 3]
        SPM_HIP_CHECK(ctx, ev.create());
        // the scratch of locate + order: keys and indices twice (the sort's in and out), scores, head flags, their sums, the
        // counts, the distinct hits.  uid and the records outlive align_run, which may grow the context's scratch: they are
        // buffers of their own.
        size_t sort_bytes = 0, scan_bytes = 0;
        SPM_HIP_CHECK(ctx, sort_pairs_tmp_bytes(ctx, n32, plan.key_bits, &sort_bytes));
        SPM_HIP_CHECK(ctx, exclusive_sum_tmp_bytes<uint32_t>(ctx, counted<uint32_t>(jloc_head_op{nullptr}), n32, &scan_bytes));
        const size_t tmp_bytes = std::max(sort_bytes, scan_bytes);
        jst_locate_params P{};
        unsigned long long *keys = nullptr; // (sorted; P.keys and P.idx are the sort's input)
        uint32_t *idx = nullptr, *offs = nullptr;
        uint8_t *head = nullptr, *d_tmp = nullptr;
        spm_hit *d_list = nullptr;
        scratch_layout L;
        L.take(P.keys, n);
        L.take(keys, n);
        L.take(P.idx, n);
        L.take(idx, n);
        L.take(P.score, n);
        L.take(head, n);
        L.take(offs, n);
        L.take(P.counts, 2);
        L.take(d_tmp, tmp_bytes);
        L.take(d_list, n);
        SPM_TRY(ensure_scratch(ctx, L.bytes()));
        L.bind(ctx->d_scratch);
        dev_scratch tmp;
        uint32_t *d_uid = nullptr;
        spm_aln *d_seg_alns = nullptr;
        SPM_HIP_CHECK(ctx, tmp.alloc(&d_uid, n * 4));
        SPM_HIP_CHECK(ctx, hipMalloc(&A->d_recs, n * sizeof(spm_jst_aln)));

        P.recs = reinterpret_cast<const unsigned long long *>(h->d);
        P.n = n32;
        P.hap_start = J->d_hap_start;
        P.T = J->ctx_tables();
        P.jb = J->jb;
        P.je = J->je;
        P.n_hap = J->H;
        P.n_groups = (J->H + kJstGroup - 1) / kJstGroup;
        P.window = J->window;
        P.m = ps->d_m;
        P.n_patterns = ps->n;
        P.report_begin = myers ? 0 : 1;
        P.ctx_bits = plan.ctx_bits;
        SPM_HIP_CHECK(ctx, hipMemsetAsync(P.counts, 0, 16, st));
        SPM_HIP_CHECK(ctx, hipEventRecord(ev[0], st));
        SPM_HIP_CHECK(ctx, launch_1d(ctx, jst_locate_kernel, n, P));
        SPM_HIP_CHECK(ctx, sort_pairs(ctx, d_tmp, tmp_bytes, P.keys, keys, P.idx, idx, n32, plan.key_bits));
        SPM_HIP_CHECK(ctx, launch_1d(ctx, jst_locate_heads_kernel, n, keys, idx, P.score, n32, head, P.counts));
        SPM_HIP_CHECK(ctx, exclusive_sum(ctx, d_tmp, tmp_bytes, counted<uint32_t>(jloc_head_op{head}), offs, n32));
        SPM_HIP_CHECK(ctx, launch_1d(ctx, jst_locate_emit_kernel, n, keys, idx, P.score, head, offs, n32, plan.ctx_bits, d_list, d_uid,
                                     P.counts));
        SPM_HIP_CHECK(ctx, hipEventRecord(ev[1], st));
        // the one read-back: {distinct, errors}; the context tables travel with it, once per index generation
        unsigned long long *c = ctx->h_counters;
        SPM_HIP_CHECK(ctx, hipMemcpyAsync(c, P.counts, 16, hipMemcpyDeviceToHost, st));
        SPM_TRY(J->fetch_ctx_tables());
        SPM_HIP_CHECK(ctx, hipStreamSynchronize(st));
        J->h_generation = J->generation;
        const auto t_list = clk::now();
        nk = c[0];
        const unsigned long long n_bad = c[1];
        if (n_bad || nk == 0 || nk > n) {
            SPM_SET_ERR(ctx, "spm_hip_jst_selection_align: %llu of %llu records cannot be located in the indexed blocks of "
                             "their tree (last symbol outside them, a cell that owns nothing, a position outside the owned "
                             "part of its context, or haplotypes that disagree on a shared hit's score); nothing was aligned",
                        n_bad ? n_bad : (unsigned long long)n, (unsigned long long)n);
            return SPM_E_INVALID;
        }
        // ---- the distinct segment hits, already in pool order; lo = the start of the hit's context ----
        std::vector<spm_hit> kh(nk);
        SPM_HIP_CHECK(ctx, hipMemcpyAsync(kh.data(), d_list, nk * sizeof(spm_hit), hipMemcpyDeviceToHost, st));
        SPM_HIP_CHECK(ctx, hipStreamSynchronize(st));
        const std::vector<uint64_t> &coff = J->h_ctx_off;
        std::vector<uint64_t> lo(nk);
        for (uint64_t i = 0; i < nk; ++i) {
            const spm_hit &x = kh[i];
            const uint64_t last = x.pattern >= ps->n ? ~0ull : myers ? x.pos - 1 : x.pos + (uint64_t)ps->m[x.pattern] - 1;
            if (last >= J->ctx_bytes) { // (pattern and position: the locate kernel has tested both)
                SPM_SET_ERR(ctx, "spm_hip_jst_selection_align: segment hit %llu lies outside the context buffer", (unsigned long long)i);
                return SPM_E_INVALID;
            }
            lo[i] = coff[(uint64_t)(std::upper_bound(coff.begin(), coff.begin() + (long)J->n_ctx, last) - coff.begin()) - 1];
        }
        SPM_TRY(jst_align_segments(ctx, J, ps, kh, lo, begin_only, t_list, "spm_hip_jst_selection_align", tmp, A.get(),
                                   &d_seg_alns));
        // ---- the gather: record i of the selection's device view -> alignment record i ----
        SPM_HIP_CHECK(ctx, hipEventRecord(ev[2], st));
        SPM_HIP_CHECK(ctx, launch_1d(ctx, jst_aln_gather_kernel, n, P.recs, d_uid, d_seg_alns, n32, nk, P.report_begin,
                                     reinterpret_cast<unsigned long long *>(A->d_recs)));
        SPM_HIP_CHECK(ctx, hipEventRecord(ev[3], st));
        SPM_TRY(jst_alns_download(ctx, A.get()));
        hipEventElapsedTime(&ms_locate, ev[0], ev[1]);
        hipEventElapsedTime(&ms_gather, ev[2], ev[3]);
        A->stats.ms_fanout = ms_locate + ms_gather;
    }
    const float ms_sort = jst_alns_close(A.get(), nk, myers, t_call);
    if (n)
        A->stats.ms_worklist += ms_sort; // the work list's second piece: the host order of the records
    if (spm_trace_on())
        fprintf(stderr, "[spm_hip] jst selection align: %llu kept records -> %llu segment alignments%s: locate + order %.3f ms, "
                        "begins %.3f, transcripts %.3f, gather %.3f; %.3f ms in all (work list %.3f)\n", (unsigned long long)n,
                (unsigned long long)nk, begin_only ? " (begins only)" : "", ms_locate, A->stats.ms_begin, A->stats.ms_cigar,
                ms_gather, A->stats.ms_host, A->stats.ms_worklist);
    *out = A.release();
    return SPM_OK;
}

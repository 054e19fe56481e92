// jst_collapse.hpp -- projected pan-genome alignments collapsed to one record per locus (spm_hip_jst_ref_alns_collapse;
// contract in spm_hip.h, scheme in DESIGN.md 4.6b).  gfx950.  Unit: jst_ref.hip.  It reads a spm_jst_ref_alns and makes
// the spm_jst_ref_loci (jst_handles.hpp) that every later stage reads.
//
// Records that share a projected slot share their content, so the content is compared once per distinct slot of the source
// pool, and the records are ordered afterwards:
//   (the slot stage of transcript_slots.hpp: a representative record and a number for every distinct slot, in pool order --
//   the numbering the projection gave these records' slots)
//   jst_col_key_kernel      one lane per slot: pattern << ref_bits | ref_begin (slots past the count: all ones; the sort is
//                           stable, so they stay behind the real ones)
//   (radix sort of the slots by that key: a GROUP is the slots of one (pattern, ref_begin))
//   jst_col_walk_kernel     one lane per sorted slot: jst_collapse_rank over its group -- how many slots of the group are
//                           strictly smaller under the rule, and whether an earlier slot has equal content
//   (hipcub exclusive sum of "first of its content" over the sorted slots: the loci before every group)
//   jst_col_number_kernel   one lane per sorted slot: loci of earlier groups + distinct smaller contents of its own group =
//                           the locus of the slot; the first slot of a content notes the locus's transcript
//   (hipcub exclusive sum of the loci's word counts, 64 bits: cigar_off)
//   jst_col_reckey_kernel   one lane per record: locus << 32 | haplotype, and the device map
//   (radix sort of the records by that key)
//   jst_col_mhead_kernel    heads of equal (locus, haplotype): the members; (hipcub exclusive sum: their numbers)
//   jst_col_total_kernel    loci, members and words for the one read-back that sizes the pools
//   jst_col_locus_kernel    one lane per locus: its record and its transcript
//   jst_col_member_kernel   one lane per sorted record: n_records, score, n_haplotypes (integer atomics: any order gives the
//                           same bytes), the member heads their haplotype, smallest score and the locus's member_off
// The walk is quadratic in the group times the transcript length; groups are the distinct contexts over one read locus, a
// handful.  max_run in the stats shows an input where they are not.  The scratch is laid out with scratch_layout.hpp;
// launches, sorts, sums, the read-back and the events are device_order.hpp's; what makes a record unusable (ref_aln_unusable)
// and the slot clamp are transcript_slots.hpp's.  Every table index is tested against its size before it is read.
#pragma once

#include "internal.hpp"
#include "device_order.hpp"
#include "jst_collapse_core.hpp"
#include "jst_handles.hpp"
#include "scratch_layout.hpp"
#include "transcript_slots.hpp"
#include "wave.hpp"

namespace spm_hip
{

enum { kColCntSlots = 0, kColCntBad, kColCntLoci, kColCntMembers, kColCntWords, kColCntMulti, kColCntMaxRun, kColCnts };
static_assert(kColCntSlots == kSlotCntSlots && kColCntBad == kSlotCntBad, "the slot stage writes the first two counters");

struct jst_collapse_params
{
    const spm_jst_ref_aln *recs;     // the source's device view
    uint32_t n;
    const uint32_t *ops;             // the source's pool
    uint64_t n_ops;
    uint32_t n_patterns;
    uint64_t n_ref;
    uint32_t ref_bits;
    uint32_t cap;                    // slots the per-slot tables hold: min(n, n_ops)
    uint32_t *rep;                   // [n_ops] smallest record index whose transcript starts at this word, or none
    uint32_t *sid;                   // [n_ops] exclusive sum of rep != none: the slot's number
    uint32_t *slot_rec;              // [cap] representative record of slot s
    unsigned long long *key_in;      // [cap] the group key of slot s ...
    uint32_t *idx_in;                // [cap] ... and s
    const unsigned long long *key;   // [cap] both sorted
    const uint32_t *idx;
    uint32_t *rank;                  // [cap] by sorted position: strictly smaller slots of the group
    uint32_t *glo;                   // [cap] by sorted position: where the group begins
    uint8_t *is_first;               // [cap] by sorted position: no earlier slot has this content
    const uint32_t *lsum;            // [cap] exclusive sum of is_first
    uint32_t *slot_locus;            // [cap] by slot number
    uint32_t *loc_rec;               // [cap] by locus: a record that holds its content
    uint32_t *loc_len;               // [cap] by locus: words of its transcript
    const unsigned long long *loc_off; // [cap] exclusive sum of loc_len
    unsigned long long *rkey_in;     // [n] locus << 32 | haplotype of record i ...
    uint32_t *ridx_in;               // [n] ... and i
    const unsigned long long *rkey;  // [n] both sorted
    const uint32_t *ridx;
    uint8_t *mhead;                  // [n] by sorted position: first record of its (locus, haplotype)
    const uint32_t *msum;            // [n] exclusive sum of mhead
    uint32_t *map;                   // [n] locus of record i (a buffer of the result)
    unsigned long long *counts;      // kColCnt*
    slot_tables slots() const { return slot_tables{rep, sid, slot_rec, n_ops, cap, counts}; } // (what the slot stage takes)
};

__device__ __forceinline__ jst_locus_key jcol_key(const spm_jst_ref_aln &a)
{
    jst_locus_key k;
    k.ref_begin = a.ref_begin;
    k.ref_end = a.ref_end;
    k.pattern = a.pattern;
    k.ref_score = a.ref_score;
    k.cigar_len = a.cigar_len;
    return k;
}

__global__ __launch_bounds__(256) void jst_col_key_kernel(const jst_collapse_params P)
{
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s >= P.cap)
        return;
    unsigned long long key = ~0ull;
    if (s < slot_count(P.counts, P.cap)) {
        const uint32_t r = P.slot_rec[s];
        if (r < P.n) {
            const spm_jst_ref_aln a = P.recs[r];
            key = P.ref_bits < 64 ? ((unsigned long long)a.pattern << P.ref_bits) | a.ref_begin : a.ref_begin;
        }
    }
    P.key_in[s] = key;
    P.idx_in[s] = s;
}

// the sorted slots as jst_collapse_rank reads them; a slot is usable if its representative passed the slot stage
struct jcol_view
{
    const jst_collapse_params &P;
    __device__ __forceinline__ spm_jst_ref_aln rec(uint32_t j) const
    {
        const uint32_t s = P.idx[j];
        const uint32_t r = s < P.cap ? P.slot_rec[s] : kSlotNone;
        spm_jst_ref_aln a{};
        if (r < P.n)
            a = P.recs[r];
        if (r >= P.n || ref_aln_unusable(P, a)) { // (never of a counted slot; an empty transcript reads no word)
            a = spm_jst_ref_aln{};
        }
        return a;
    }
    __device__ __forceinline__ jst_locus_key key(uint32_t j) const { return jcol_key(rec(j)); }
    __device__ __forceinline__ const uint32_t *words(uint32_t j) const { return P.ops + rec(j).cigar_off; }
};

__global__ __launch_bounds__(256) void jst_col_walk_kernel(const jst_collapse_params P)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const uint32_t n_slots = slot_count(P.counts, P.cap);
    if (i >= n_slots)
        return;
    const unsigned long long key = P.key[i];
    uint32_t lo = i, hi = i + 1;
    while (lo > 0 && P.key[lo - 1] == key)
        --lo;
    while (hi < n_slots && P.key[hi] == key)
        ++hi;
    const jcol_view V{P};
    const jst_collapse_rank_result R = jst_collapse_rank(V, lo, hi, i);
    P.rank[i] = R.smaller;
    P.glo[i] = lo;
    P.is_first[i] = R.first == i ? 1 : 0;
    if (R.first == i && R.n_equal > 1)
        atomicAdd(&P.counts[kColCntMulti], 1ull);
    atomicMax(&P.counts[kColCntMaxRun], (unsigned long long)R.n_tuple);
}

__global__ __launch_bounds__(256) void jst_col_number_kernel(const jst_collapse_params P)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const uint32_t n_slots = slot_count(P.counts, P.cap);
    if (i >= n_slots)
        return;
    const uint32_t lo = P.glo[i], rank = P.rank[i];
    uint32_t below = 0;
    for (uint32_t j = lo; j < n_slots && P.glo[j] == lo; ++j)
        below += (P.is_first[j] && P.rank[j] < rank) ? 1u : 0u;
    const uint32_t locus = P.lsum[lo] + below;
    const uint32_t s = P.idx[i];
    if (s < P.cap && locus < P.cap) {
        P.slot_locus[s] = locus;
        if (P.is_first[i]) {
            const uint32_t r = P.slot_rec[s];
            P.loc_rec[locus] = r;
            P.loc_len[locus] = r < P.n ? P.recs[r].cigar_len : 0u;
        }
    }
    if (i == n_slots - 1)
        P.counts[kColCntLoci] = (unsigned long long)P.lsum[i] + P.is_first[i];
}

__global__ __launch_bounds__(256) void jst_col_reckey_kernel(const jst_collapse_params P)
{
    const unsigned long long i = blockIdx.x * 256ull + threadIdx.x;
    bool bad = false;
    if (i < P.n) {
        const spm_jst_ref_aln a = P.recs[i];
        uint32_t locus = kSlotNone;
        if (!ref_aln_unusable(P, a)) {
            const uint32_t s = P.sid[a.cigar_off];
            const uint32_t r = s < P.cap ? P.slot_rec[s] : kSlotNone;
            // a record must say what the representative of its slot says: the content was compared through that one
            if (r < P.n && jst_collapse_cmp_tuple(jcol_key(P.recs[r]), jcol_key(a)) == 0 && P.recs[r].cigar_off == a.cigar_off)
                locus = P.slot_locus[s];
        }
        bad = locus >= P.cap;
        P.map[i] = bad ? kSlotNone : locus;
        P.rkey_in[i] = bad ? ~0ull : ((unsigned long long)locus << 32) | a.haplotype;
        P.ridx_in[i] = (uint32_t)i;
    }
    count_flagged(&P.counts[kColCntBad], bad);
}

__global__ __launch_bounds__(256) void jst_col_mhead_kernel(const jst_collapse_params P)
{
    const unsigned long long j = blockIdx.x * 256ull + threadIdx.x;
    if (j < P.n)
        P.mhead[j] = (j == 0 || P.rkey[j] != P.rkey[j - 1]) ? 1 : 0;
}

__global__ void jst_col_total_kernel(const jst_collapse_params P)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const uint32_t n_loci = (uint32_t)min(P.counts[kColCntLoci], (unsigned long long)P.cap);
        P.counts[kColCntWords] = n_loci ? P.loc_off[n_loci - 1] + P.loc_len[n_loci - 1] : 0ull;
        P.counts[kColCntMembers] = P.n ? (unsigned long long)P.msum[P.n - 1] + P.mhead[P.n - 1] : 0ull;
    }
}

// the buffers of the result, sized by the read-back
struct jst_collapse_out
{
    spm_jst_ref_locus *loci;
    uint32_t n_loci;
    uint32_t *ops;
    uint64_t n_ops;
    uint32_t *members;
    int32_t *member_scores;
    uint32_t n_members;
};

__global__ __launch_bounds__(256) void jst_col_locus_kernel(const jst_collapse_params P, const jst_collapse_out O)
{
    const uint32_t l = blockIdx.x * 256u + threadIdx.x;
    bool bad = false;
    if (l < O.n_loci) {
        const uint32_t r = P.loc_rec[l];
        const unsigned long long off = P.loc_off[l];
        spm_jst_ref_aln a{};
        bad = r >= P.n;
        if (!bad) {
            a = P.recs[r];
            bad = ref_aln_unusable(P, a) || a.cigar_len != P.loc_len[l] || off + a.cigar_len > O.n_ops;
        }
        spm_jst_ref_locus o{};
        o.score = 0x7FFFFFFF;
        if (!bad) {
            o.ref_begin = a.ref_begin;
            o.ref_end = a.ref_end;
            o.pattern = a.pattern;
            o.ref_score = a.ref_score;
            o.cigar_off = (uint32_t)off;
            o.cigar_len = a.cigar_len;
            for (uint32_t w = 0; w < a.cigar_len; ++w)
                O.ops[off + w] = P.ops[a.cigar_off + w];
        }
        O.loci[l] = o;
    }
    count_flagged(&P.counts[kColCntBad], bad);
}

__global__ __launch_bounds__(256) void jst_col_member_kernel(const jst_collapse_params P, const jst_collapse_out O)
{
    const unsigned long long j = blockIdx.x * 256ull + threadIdx.x;
    bool bad = false;
    if (j < P.n) {
        const unsigned long long key = P.rkey[j];
        const uint32_t locus = (uint32_t)(key >> 32), i = P.ridx[j];
        const uint32_t head = P.mhead[j];
        const uint32_t mi = P.msum[j] + head - 1u; // (msum[0] = 0 and mhead[0] = 1: never wraps)
        bad = locus >= O.n_loci || i >= P.n || mi >= O.n_members;
        if (!bad) {
            spm_jst_ref_locus *L = &O.loci[locus];
            const int32_t score = P.recs[i].score;
            atomicAdd(&L->n_records, 1u);
            atomicMin(&L->score, score);
            if (head) {
                int32_t best = score;
                for (unsigned long long jj = j + 1; jj < P.n && P.rkey[jj] == key; ++jj) {
                    const uint32_t ii = P.ridx[jj];
                    if (ii < P.n)
                        best = min(best, P.recs[ii].score);
                }
                O.members[mi] = (uint32_t)key;
                O.member_scores[mi] = best;
                atomicAdd(&L->n_haplotypes, 1u);
                if (j == 0 || (uint32_t)(P.rkey[j - 1] >> 32) != locus)
                    L->member_off = mi;
            }
        }
    }
    count_flagged(&P.counts[kColCntBad], bad);
}

} // namespace spm_hip

extern "C" void spm_hip_jst_ref_loci_destroy(spm_jst_ref_loci *l)
{
    if (!l)
        return;
    if (l->ctx && (l->d_loci || l->d_ops || l->d_members || l->d_map || l->d_member_scores))
        hipStreamSynchronize(l->ctx->stream);
    hipFree(l->d_loci);
    hipFree(l->d_ops);
    hipFree(l->d_members);
    hipFree(l->d_member_scores);
    hipFree(l->d_map);
    delete l;
}

extern "C" int spm_hip_jst_ref_alns_collapse(spm_jst_ref_alns *a, uint32_t flags, spm_jst_ref_loci **out)
{
    using namespace spm_hip;
    if (!a || !out)
        return SPM_E_INVALID;
    spm_ctx *ctx = a->ctx;
    const auto t_call = clk::now();
    if (flags) {
        SPM_SET_ERR(ctx, "spm_hip_jst_ref_alns_collapse: unknown flag bits 0x%x", flags);
        return SPM_E_INVALID;
    }
    const jst_collapse_plan plan = plan_jst_collapse(a->n_patterns, a->n_ref); // decided before any launch
    if (!plan.ok) {
        SPM_SET_ERR(ctx, "spm_hip_jst_ref_alns_collapse: needle index and reference position do not fit one 64-bit key "
                         "(%u + %u bits)", plan.pat_bits, plan.ref_bits);
        return SPM_E_UNSUPPORTED;
    }
    const uint64_t n = a->n, n_src_ops = a->n_ops;
    if (n > 0xFFFFFFFFull) {
        SPM_SET_ERR(ctx, "spm_hip_jst_ref_alns_collapse: more than 2^32 - 1 records");
        return SPM_E_UNSUPPORTED;
    }
    SPM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    std::unique_ptr<spm_jst_ref_loci, void (*)(spm_jst_ref_loci *)> R(new spm_jst_ref_loci, spm_hip_jst_ref_loci_destroy);
    R->ctx = ctx;
    R->n_alns = n;
    R->stats.n_alns = n;
    hipStream_t st = ctx->stream;
    float ms_slots = 0, ms_order = 0, ms_records = 0, ms_emit = 0;
    if (n) {
        if (n_src_ops == 0 || !a->d_ops || !a->d_recs || a->host.size() != n) {
            SPM_SET_ERR(ctx, "spm_hip_jst_ref_alns_collapse: %llu records but no transcript pool or no host view",
                        (unsigned long long)n);
            return SPM_E_INVALID;
        }
        const uint32_t n32 = (uint32_t)n;
        const uint32_t cap = (uint32_t)std::min<uint64_t>(n, n_src_ops);
        const uint32_t slot_key_bits = std::max(1u, plan.pat_bits + plan.ref_bits);
        const uint32_t rec_key_bits = 32u + std::max(1u, jst_collapse_bits(cap - 1));
        hip_events<6> ev;
        SPM_HIP_CHECK(ctx, ev.create());
        size_t b[5] = {};
        SPM_HIP_CHECK(ctx, slot_stage_tmp_bytes(ctx, n_src_ops, &b[0]));
        SPM_HIP_CHECK(ctx, exclusive_sum_tmp_bytes<uint32_t>(ctx, counted<uint32_t>(byte_op{nullptr}), std::max(n32, cap), &b[1]));
        SPM_HIP_CHECK(ctx, exclusive_sum_tmp_bytes<unsigned long long>(ctx, counted<unsigned long long>(widen_op{nullptr}), cap,
                                                                       &b[2]));
        SPM_HIP_CHECK(ctx, sort_pairs_tmp_bytes(ctx, cap, slot_key_bits, &b[3]));
        SPM_HIP_CHECK(ctx, sort_pairs_tmp_bytes(ctx, n32, rec_key_bits, &b[4]));
        const size_t tmp_bytes = *std::max_element(b, b + 5);
        jst_collapse_params P{};
        // (what the sorts and the sums write; the kernels read them through P's pointers to const)
        unsigned long long *d_key = nullptr, *d_loff = nullptr, *d_rkey = nullptr;
        uint32_t *d_idx = nullptr, *d_lsum = nullptr, *d_ridx = nullptr, *d_msum = nullptr;
        uint8_t *d_tmp = nullptr;
        scratch_layout L;
        L.take(P.rep, n_src_ops);
        L.take(P.sid, n_src_ops);
        L.take(P.slot_rec, cap);
        L.take(P.key_in, cap);
        L.take(d_key, cap);
        L.take(P.idx_in, cap);
        L.take(d_idx, cap);
        L.take(P.rank, cap);
        L.take(P.glo, cap);
        L.take(P.is_first, cap);
        L.take(d_lsum, cap);
        L.take(P.slot_locus, cap);
        L.take(P.loc_rec, cap);
        L.take(P.loc_len, cap);
        L.take(d_loff, cap);
        L.take(P.rkey_in, n);
        L.take(d_rkey, n);
        L.take(P.ridx_in, n);
        L.take(d_ridx, n);
        L.take(P.mhead, n);
        L.take(d_msum, n);
        L.take(P.counts, kColCnts);
        L.take(d_tmp, tmp_bytes);
        SPM_TRY(ensure_scratch(ctx, L.bytes()));
        L.bind(ctx->d_scratch);
        SPM_HIP_CHECK(ctx, hipMalloc(&R->d_map, n * 4));

        P.recs = a->d_recs;
        P.n = n32;
        P.ops = a->d_ops;
        P.n_patterns = a->n_patterns;
        P.n_ref = a->n_ref;
        P.ref_bits = plan.ref_bits;
        P.n_ops = n_src_ops;
        P.cap = cap;
        P.key = d_key;
        P.idx = d_idx;
        P.lsum = d_lsum;
        P.loc_off = d_loff;
        P.rkey = d_rkey;
        P.ridx = d_ridx;
        P.msum = d_msum;
        P.map = R->d_map;
        // ---- slots: one representative per distinct slot of the source pool, numbered in pool order ----
        SPM_HIP_CHECK(ctx, hipMemsetAsync(P.counts, 0, kColCnts * 8, st));
        SPM_HIP_CHECK(ctx, hipEventRecord(ev[0], st));
        SPM_HIP_CHECK(ctx, slot_stage_enqueue(ctx, P.recs, n32, P.slots(), ref_aln_unusable_op{{P.n_ops, P.n_patterns, P.n_ref}},
                                              d_tmp, tmp_bytes));
        SPM_HIP_CHECK(ctx, hipEventRecord(ev[1], st));
        // ---- order: groups of one (pattern, ref_begin), the rule inside a group, the locus of every slot ----
        SPM_HIP_CHECK(ctx, hipMemsetAsync(P.is_first, 0, cap, st));
        SPM_HIP_CHECK(ctx, hipMemsetAsync(P.loc_len, 0, (size_t)cap * 4, st));
        SPM_HIP_CHECK(ctx, hipMemsetAsync(P.slot_locus, 0xFF, (size_t)cap * 4, st));
        SPM_HIP_CHECK(ctx, launch_1d(ctx, jst_col_key_kernel, cap, P));
        SPM_HIP_CHECK(ctx, sort_pairs(ctx, d_tmp, tmp_bytes, P.key_in, d_key, P.idx_in, d_idx, cap, slot_key_bits));
        SPM_HIP_CHECK(ctx, launch_1d(ctx, jst_col_walk_kernel, cap, P));
        SPM_HIP_CHECK(ctx, exclusive_sum(ctx, d_tmp, tmp_bytes, counted<uint32_t>(byte_op{P.is_first}), d_lsum, cap));
        SPM_HIP_CHECK(ctx, launch_1d(ctx, jst_col_number_kernel, cap, P));
        SPM_HIP_CHECK(ctx, exclusive_sum(ctx, d_tmp, tmp_bytes, counted<unsigned long long>(widen_op{P.loc_len}), d_loff, cap));
        SPM_HIP_CHECK(ctx, hipEventRecord(ev[2], st));
        // ---- records: (locus, haplotype) order, the member heads ----
        SPM_HIP_CHECK(ctx, launch_1d(ctx, jst_col_reckey_kernel, n, P));
        SPM_HIP_CHECK(ctx, sort_pairs(ctx, d_tmp, tmp_bytes, P.rkey_in, d_rkey, P.ridx_in, d_ridx, n32, rec_key_bits));
        SPM_HIP_CHECK(ctx, launch_1d(ctx, jst_col_mhead_kernel, n, P));
        SPM_HIP_CHECK(ctx, exclusive_sum(ctx, d_tmp, tmp_bytes, counted<uint32_t>(byte_op{P.mhead}), d_msum, n32));
        SPM_HIP_CHECK(ctx, launch_1d<64>(ctx, jst_col_total_kernel, 1, P));
        SPM_HIP_CHECK(ctx, hipEventRecord(ev[3], st));
        // the one read-back that sizes the pools
        SPM_HIP_CHECK(ctx, read_counts(ctx, P.counts, kColCnts));
        unsigned long long *c = ctx->h_counters;
        const unsigned long long n_slots = c[kColCntSlots], n_bad = c[kColCntBad], n_loci = c[kColCntLoci],
                                 n_members = c[kColCntMembers], total = c[kColCntWords];
        if (n_bad || n_slots == 0 || n_slots > cap || n_loci == 0 || n_loci > n_slots || n_members < n_loci || n_members > n ||
            total > n_src_ops) {
            SPM_SET_ERR(ctx, "spm_hip_jst_ref_alns_collapse: %llu records cannot be collapsed (a transcript outside the pool, a "
                             "needle or a range outside the tree, or a record that disagrees with its slot); nothing was "
                             "collapsed", n_bad ? n_bad : (unsigned long long)n);
            return SPM_E_INVALID;
        }
        R->n = n_loci;
        R->n_ops = total;
        R->n_members = n_members;
        SPM_HIP_CHECK(ctx, hipMalloc(&R->d_loci, n_loci * sizeof(spm_jst_ref_locus)));
        SPM_HIP_CHECK(ctx, hipMalloc(&R->d_ops, std::max<uint64_t>(total, 1) * 4));
        SPM_HIP_CHECK(ctx, hipMalloc(&R->d_members, n_members * 4));
        SPM_HIP_CHECK(ctx, hipMalloc(&R->d_member_scores, n_members * 4));
        jst_collapse_out O{R->d_loci, (uint32_t)n_loci, R->d_ops, total, R->d_members, R->d_member_scores, (uint32_t)n_members};
        // ---- emit: the loci and their transcripts, then what the records add to them ----
        SPM_HIP_CHECK(ctx, hipEventRecord(ev[4], st));
        SPM_HIP_CHECK(ctx, launch_1d(ctx, jst_col_locus_kernel, n_loci, P, O));
        SPM_HIP_CHECK(ctx, launch_1d(ctx, jst_col_member_kernel, n, P, O));
        SPM_HIP_CHECK(ctx, hipEventRecord(ev[5], st));
        // ---- the host view: a plain download; the host map goes through the slot tables ----
        slot_host_map slot(n_src_ops);
        std::vector<uint32_t> sloc(n_slots);
        R->host.resize(n_loci);
        R->host_ops.resize(total);
        R->host_members.resize(n_members);
        R->host_member_scores.resize(n_members);
        SPM_HIP_CHECK(ctx, hipMemcpyAsync(c, P.counts, kColCnts * 8, hipMemcpyDeviceToHost, st));
        SPM_HIP_CHECK(ctx, slot.download(ctx, P.slots()));
        SPM_HIP_CHECK(ctx, hipMemcpyAsync(sloc.data(), P.slot_locus, n_slots * 4, hipMemcpyDeviceToHost, st));
        SPM_HIP_CHECK(ctx, hipMemcpyAsync(R->host.data(), R->d_loci, n_loci * sizeof(spm_jst_ref_locus), hipMemcpyDeviceToHost, st));
        if (total)
            SPM_HIP_CHECK(ctx, hipMemcpyAsync(R->host_ops.data(), R->d_ops, total * 4, hipMemcpyDeviceToHost, st));
        SPM_HIP_CHECK(ctx, hipMemcpyAsync(R->host_members.data(), R->d_members, n_members * 4, hipMemcpyDeviceToHost, st));
        SPM_HIP_CHECK(ctx, hipMemcpyAsync(R->host_member_scores.data(), R->d_member_scores, n_members * 4, hipMemcpyDeviceToHost, st));
        SPM_HIP_CHECK(ctx, hipStreamSynchronize(st));
        hipEventElapsedTime(&ms_slots, ev[0], ev[1]);
        hipEventElapsedTime(&ms_order, ev[1], ev[2]);
        hipEventElapsedTime(&ms_records, ev[2], ev[3]);
        hipEventElapsedTime(&ms_emit, ev[4], ev[5]);
        if (c[kColCntBad]) {
            SPM_SET_ERR(ctx, "spm_hip_jst_ref_alns_collapse: %llu loci or members came out of the emit stage differently from "
                             "the count", c[kColCntBad]);
            return SPM_E_INVALID;
        }
        R->host_map.resize(n);
        for (uint64_t i = 0; i < n; ++i) {
            const spm_jst_ref_aln &x = a->host[i];
            const uint32_t s = slot.of(x.cigar_off);
            if (s >= n_slots || sloc[s] >= n_loci) {
                SPM_SET_ERR(ctx, "spm_hip_jst_ref_alns_collapse: host record %llu names no locus", (unsigned long long)i);
                return SPM_E_INVALID;
            }
            R->host_map[i] = sloc[s];
        }
        R->stats.n_slots = n_slots;
        R->stats.n_multi_slot = c[kColCntMulti];
        R->stats.max_run = c[kColCntMaxRun];
    }
    R->stats.ms_slots = ms_slots;
    R->stats.ms_order = ms_order;
    R->stats.ms_records = ms_records;
    R->stats.ms_emit = ms_emit;
    R->stats.ms_total = ms_slots + ms_order + ms_records + ms_emit;
    R->stats.n_loci = R->n;
    R->stats.n_members = R->n_members;
    R->stats.n_ops = R->n_ops;
    R->stats.ms_host = ms_since(t_call);
    if (spm_trace_on())
        fprintf(stderr, "[spm_hip] jst collapse: %llu records, %llu slots -> %llu loci, %llu members, %llu words (%llu loci merge "
                        "slots, longest run %llu): slots %.3f ms, order %.3f, records %.3f, emit %.3f; %.3f ms in all\n",
                (unsigned long long)n, (unsigned long long)R->stats.n_slots, (unsigned long long)R->n,
                (unsigned long long)R->n_members, (unsigned long long)R->n_ops, (unsigned long long)R->stats.n_multi_slot,
                (unsigned long long)R->stats.max_run, ms_slots, ms_order, ms_records, ms_emit, R->stats.ms_host);
    *out = R.release();
    return SPM_OK;
}

extern "C" int spm_hip_jst_ref_loci_view(spm_jst_ref_loci *l, const spm_jst_ref_locus **records, uint64_t *n, const uint32_t **ops,
                                         uint64_t *n_ops, const uint32_t **members, const int32_t **member_scores,
                                         uint64_t *n_members)
{
    if (!l)
        return SPM_E_INVALID;
    return pool_out(pool_src<spm_jst_ref_locus>{l->host.data(), l->n, l->host_ops.data(), l->n_ops, l->host_members.data(),
                                                l->host_member_scores.data(), l->n_members},
                    records, n, ops, n_ops, members, member_scores, n_members);
}

extern "C" int spm_hip_jst_ref_loci_device(spm_jst_ref_loci *l, const void **records, uint64_t *n, const void **ops, uint64_t *n_ops,
                                           const void **members, const void **member_scores, uint64_t *n_members)
{
    if (!l)
        return SPM_E_INVALID;
    return pool_out(pool_src<void, void, void>{l->d_loci, l->n, l->d_ops, l->n_ops, l->d_members, l->d_member_scores,
                                               l->n_members},
                    records, n, ops, n_ops, members, member_scores, n_members);
}

extern "C" int spm_hip_jst_ref_loci_map(spm_jst_ref_loci *l, const uint32_t **host_map, const void **device_map, uint64_t *n_alns)
{
    if (!l || !n_alns)
        return SPM_E_INVALID;
    if (host_map)
        *host_map = l->host_map.data();
    if (device_map)
        *device_map = l->d_map;
    *n_alns = l->n_alns;
    return SPM_OK;
}

extern "C" int spm_hip_jst_ref_loci_stats(const spm_jst_ref_loci *l, spm_jst_collapse_stats *out)
{
    if (!l || !out)
        return SPM_E_INVALID;
    *out = l->stats;
    return SPM_OK;
}

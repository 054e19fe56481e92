// jst_rescue.hpp -- mate rescue (spm_hip_jst_pairs_rescue; contract in spm_hip.h, scheme in DESIGN.md 4.10, the rule in
// jst_rescue_core.hpp).  gfx950.  Unit: jst_reads.hip.  It reads the loci, the read summary and the pairs (jst_handles.hpp).
//   jst_rescue_jobs_kernel<kEmit>   one lane per pair: reads the pair record, both read records and the anchor loci, tests
//                                   them (jst_rescue_pair_ok: every index before it is one) and, first, counts the pair's 0, 1
//                                   or 2 jobs; an exclusive sum later, the same lanes write the job descriptors in pair order;
//   jst_rescue_search_kernel<NW>    one wave per job, four jobs per workgroup, NW = ceil(m / 64) words.  The wave builds the
//                                   needle's forward match masks [sigma][NW] in LDS by ballots over the ranks of the
//                                   alignment tables; lane i scans chunk i of the job's admissible ends, cold from
//                                   max(lo, first end - 1 - (m + k)), with the NW words in registers, and keeps the minimal
//                                   (uint32) d << 32 | (e - lo); a wave-wide minimum by shuffles, and lane 0 writes it.  No
//                                   atomics.  A launch takes the jobs of its own NW and leaves the others alone;
//   jst_rescue_emit_kernel          one lane per job: the record (classification, tlen, flag: jst_rescue_record) from the job
//                                   and, for a found one, the begin and the transcript align_run left; statistics by
//                                   count_flagged.
// Begins and transcripts are those of spm_hip_hits_align: the host builds the align_work from the found jobs' (pattern, e, d,
// lo) and align_run (align.hip) writes them on the device.  The job list outlives align_run, which may grow the context's
// scratch: it is an allocation of its own.
#pragma once

#include <hip/hip_runtime.h>

#include "internal.hpp"
#include "device_order.hpp"
#include "jst_handles.hpp"
#include "jst_rescue_core.hpp"
#include "scratch_layout.hpp"
#include "wave.hpp"

namespace spm_hip
{

enum {
    kRescueCntBad = 0,
    kRescueCntJobs,
    kRescueCntMaxWindow,
    kRescueCntRescued,
    kRescueCntNone,
    kRescueCntNotConcordant,
    kRescueCntShort,
    kRescueCnts
};

struct jst_rescue_job // 40 bytes
{
    uint64_t lo;      // the window's first symbol: no alignment begins left of it
    uint64_t e_first; // admissible ends [e_first, e_first + n_ends)
    uint32_t n_ends;
    uint32_t pattern; // the needle
    uint32_t pair;
    uint32_t anchor;  // locus index, tested against the loci
    uint64_t key;     // the candidate (jst_rescue_key), kJstRescueNoKey: none
};
static_assert(sizeof(jst_rescue_job) == 40, "jst_rescue_job layout");

struct jst_rescue_params
{
    const spm_jst_ref_locus *loci = nullptr;
    uint32_t n = 0;                      // loci
    const spm_jst_read *reads = nullptr; // [2 n_pairs]
    const spm_jst_pair *pairs = nullptr; // [n_pairs]
    uint32_t n_pairs = 0;
    const uint8_t *text = nullptr;       // the reference's ranks
    uint64_t N = 0;
    uint32_t sigma = 4;
    const uint8_t *ranks = nullptr;      // needle ranks, needle p = ranks[offsets[p] ..) (the set's alignment tables)
    const uint32_t *offsets = nullptr;
    const int32_t *m = nullptr;          // [4 n_pairs at least]
    uint32_t min_tlen = 0, max_tlen = 0, k = 0;
    uint32_t *cnt = nullptr;             // [n_pairs] jobs of every pair
    uint32_t *offs = nullptr;            // [n_pairs] their exclusive sum
    jst_rescue_job *jobs = nullptr;      // [n_jobs]
    uint32_t n_jobs = 0;
    const uint32_t *aln_of = nullptr;    // [n_jobs] found jobs: their record among alns
    const spm_aln *alns = nullptr;       // [n_alns]
    uint32_t n_alns = 0;
    spm_jst_rescue *out = nullptr;       // [n_jobs]
    unsigned long long *counts = nullptr; // [kRescueCnts]
};

template <bool kEmit> __global__ __launch_bounds__(256) void jst_rescue_jobs_kernel(const jst_rescue_params P)
{
    const unsigned long long p = blockIdx.x * 256ull + threadIdx.x;
    uint32_t anchors = 0, window = 0;
    bool bad = false;
    if (p < P.n_pairs) {
        const spm_jst_pair R = P.pairs[p];
        bad = !jst_rescue_pair_ok(P.loci, P.n, P.reads[2 * p], P.reads[2 * p + 1], R, (uint32_t)p, P.N);
        anchors = bad ? 0u : jst_rescue_anchors(R);
        if (!kEmit) {
            P.cnt[p] = jst_rescue_job_count(anchors);
        } else {
            uint32_t at = P.offs[p];
            for (int x = 1; x >= 0; --x) { // (the job anchored at mate 2 rescues mate 1: it comes first)
                if (!(anchors >> x & 1u))
                    continue;
                const uint32_t a = x ? R.locus2 : R.locus1;
                const spm_jst_ref_locus A = P.loci[a]; // (a < n, A.ref_begin <= A.ref_end <= N: jst_rescue_pair_ok)
                jst_rescue_job J;
                J.pattern = jst_rescue_needle((uint32_t)p, (uint32_t)x, A.pattern);
                const uint32_t m = (uint32_t)P.m[J.pattern];
                const jst_rescue_window W = jst_rescue_window_of(A.ref_begin, A.ref_end, (A.pattern & 1u) != 0, P.min_tlen, P.max_tlen, P.N);
                J.lo = W.lo;
                J.e_first = W.e_first;
                J.n_ends = m <= P.k ? 0u : W.n_ends; // (a needle of m <= k symbols is not searched)
                J.pair = (uint32_t)p;
                J.anchor = a;
                J.key = kJstRescueNoKey;
                if (at < P.n_jobs)
                    P.jobs[at] = J;
                ++at;
                const uint32_t w = (uint32_t)(W.hi - W.lo);
                window = w > window ? w : window;
            }
        }
    }
    if (!kEmit) {
        count_flagged(&P.counts[kRescueCntBad], bad);
        count_flagged(&P.counts[kRescueCntJobs], (anchors & 1u) != 0);
        count_flagged(&P.counts[kRescueCntJobs], (anchors & 2u) != 0);
    } else {
        window = wave_max(window);
        if ((threadIdx.x & 63) == 0 && window)
            atomicMax(&P.counts[kRescueCntMaxWindow], (unsigned long long)window);
    }
}

// dynamic LDS: 4 waves x sigma x NW match masks
template <int NW> __global__ __launch_bounds__(256) void jst_rescue_search_kernel(const jst_rescue_params P)
{
    extern __shared__ uint64_t rescue_lds[];
    const uint32_t wv = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    const unsigned long long j = blockIdx.x * 4ull + wv;
    if (j >= P.n_jobs)
        return; // (whole waves: j is uniform across the wave, and no workgroup barrier follows)
    const jst_rescue_job J = P.jobs[j];
    const uint32_t m = (uint32_t)P.m[J.pattern];
    if ((m + 63) / 64 != (uint32_t)NW || J.n_ends == 0)
        return; // (another launch's job, or nothing to search: the key stays kJstRescueNoKey)
    uint64_t *masks = rescue_lds + (size_t)wv * P.sigma * NW;
    const uint8_t *needle = P.ranks + P.offsets[J.pattern];
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        const uint32_t i = (uint32_t)w * 64u + lane;
        const uint32_t c = i < m ? needle[i] : 0xFFFFu;
        for (uint32_t r = 0; r < P.sigma; ++r) {
            const unsigned long long eq = __ballot(c == r);
            if (lane == 0)
                masks[r * NW + w] = eq;
        }
    }
    // lane 0's LDS writes before every lane's LDS reads: one wave, whose LDS operations complete in order
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    jst_rescue_window W;
    W.lo = J.lo;
    W.e_first = J.e_first;
    W.n_ends = J.n_ends;
    const jst_rescue_chunk C = jst_rescue_chunk_of(W, lane, m, P.k);
    uint64_t key = jst_rescue_chunk_scan<NW>(masks, P.sigma, m, P.k, P.text, C, J.lo);
    for (int d = 32; d; d >>= 1) {
        const uint64_t k2 = __shfl_xor(key, d);
        key = k2 < key ? k2 : key;
    }
    if (lane == 0)
        P.jobs[j].key = key;
}

__global__ __launch_bounds__(256) void jst_rescue_emit_kernel(const jst_rescue_params P)
{
    const unsigned long long j = blockIdx.x * 256ull + threadIdx.x;
    bool bad = false, rescued = false, none = false, not_concordant = false, is_short = false;
    if (j < P.n_jobs) {
        const jst_rescue_job J = P.jobs[j];
        const spm_jst_ref_locus A = P.loci[J.anchor]; // (tested by jst_rescue_jobs_kernel)
        const bool found = J.key != kJstRescueNoKey;
        spm_aln X{};
        if (found) {
            const uint32_t a = P.aln_of[j];
            bad = a >= P.n_alns;
            if (!bad)
                X = P.alns[a];
        }
        spm_jst_rescue O{};
        if (!bad) {
            O = jst_rescue_record(A, J.anchor, J.pair, (A.pattern >> 1) & 1u, J.pattern, found, X.begin, X.end, X.score, X.cigar_off,
                                  X.cigar_len, P.min_tlen, P.max_tlen);
            rescued = O.status == SPM_RESCUE_RESCUED;
            none = O.status == SPM_RESCUE_NONE;
            not_concordant = O.status == SPM_RESCUE_NOT_CONCORDANT;
            is_short = (uint32_t)P.m[J.pattern] <= P.k;
        }
        P.out[j] = O;
    }
    count_flagged(&P.counts[kRescueCntBad], bad);
    count_flagged(&P.counts[kRescueCntRescued], rescued);
    count_flagged(&P.counts[kRescueCntNone], none);
    count_flagged(&P.counts[kRescueCntNotConcordant], not_concordant);
    count_flagged(&P.counts[kRescueCntShort], is_short);
}

struct rescue_cnt_op
{
    const uint32_t *cnt;
    __host__ __device__ uint32_t operator()(uint32_t i) const { return cnt[i]; }
};

template <int NW> hipError_t rescue_search_launch(spm_ctx *ctx, const jst_rescue_params &P)
{
    const size_t lds = (size_t)4 * P.sigma * NW * sizeof(uint64_t);
    hipLaunchKernelGGL(jst_rescue_search_kernel<NW>, dim3((P.n_jobs + 3) / 4), dim3(256), lds, ctx->stream, P);
    return hipGetLastError();
}

} // namespace spm_hip

extern "C" void spm_hip_jst_rescues_destroy(spm_jst_rescues *r)
{
    if (!r)
        return;
    if (r->ctx && (r->d || r->d_ops))
        hipStreamSynchronize(r->ctx->stream);
    hipFree(r->d_ops);
    r->d_ops = nullptr;
    hipFree(r->d);
    delete r;
}

extern "C" int spm_hip_jst_pairs_rescue(spm_jst_ref_loci *l, spm_jst_reads *r, spm_jst_pairs *pr, const spm_text *ref,
                                        const spm_patterns *ps, const spm_jst_rescue_opts *opts, spm_jst_rescues **out)
{
    using namespace spm_hip;
    static const char *const who = "spm_hip_jst_pairs_rescue";
    if (!l || !out)
        return SPM_E_INVALID;
    spm_ctx *ctx = l->ctx;
    const auto t_call = clk::now();
    if (!r || !pr || !ref || !ps || !opts) {
        SPM_SET_ERR(ctx, "%s: NULL %s", who, !r ? "reads handle" : !pr ? "pairs handle" : !ref ? "reference" : !ps ? "patterns" : "opts");
        return SPM_E_INVALID;
    }
    if (opts->flags || opts->reserved) {
        SPM_SET_ERR(ctx, "%s: unknown flag bits 0x%x or reserved %u, both must be 0", who, opts->flags, opts->reserved);
        return SPM_E_INVALID;
    }
    if (!jst_rescue_opts_ok(*opts)) {
        SPM_SET_ERR(ctx, "%s: min_tlen %u, max_tlen %u: not 1 <= min_tlen <= max_tlen <= 2^31 - 1", who, opts->min_tlen, opts->max_tlen);
        return SPM_E_INVALID;
    }
    if (r->ctx != ctx || pr->ctx != ctx || ref->ctx != ctx || ps->ctx != ctx) {
        SPM_SET_ERR(ctx, "%s: the %s belongs to another context", who,
                    r->ctx != ctx ? "reads handle" : pr->ctx != ctx ? "pairs handle" : ref->ctx != ctx ? "reference" : "needle set");
        return SPM_E_INVALID;
    }
    if (r->strands != 2) {
        SPM_SET_ERR(ctx, "%s: the reads handle was made with strands == %u, mates need a stranded set (2)", who, r->strands);
        return SPM_E_INVALID;
    }
    if ((r->n & 1) || pr->n != r->n / 2) {
        SPM_SET_ERR(ctx, "%s: %llu pairs do not belong to %llu reads", who, (unsigned long long)pr->n, (unsigned long long)r->n);
        return SPM_E_INVALID;
    }
    if (r->n_loci != l->n) {
        SPM_SET_ERR(ctx, "%s: the reads handle was made from %llu loci, these are %llu", who, (unsigned long long)r->n_loci,
                    (unsigned long long)l->n);
        return SPM_E_INVALID;
    }
    if (ps->algo == SPM_ALGO_MYERS_PREFIX) {
        SPM_SET_ERR(ctx, "%s: a MYERS_PREFIX needle set cannot be aligned (not supported)", who);
        return SPM_E_UNSUPPORTED;
    }
    if (ps->algo != SPM_ALGO_MYERS || ps->strands != 2 || (uint64_t)ps->n != 2 * r->n) {
        SPM_SET_ERR(ctx, "%s: the needle set is not the stranded Myers set of these %llu reads (algo %d, strands %u, %u needles)", who,
                    (unsigned long long)r->n, ps->algo, ps->strands, ps->n);
        return SPM_E_INVALID;
    }
    if (ps->max_m > kJstRescueMaxM) {
        SPM_SET_ERR(ctx, "%s: a needle of %u symbols: above %u is not supported", who, ps->max_m, kJstRescueMaxM);
        return SPM_E_UNSUPPORTED;
    }
    if (ref->sigma != ps->sigma) {
        SPM_SET_ERR(ctx, "%s: the reference has sigma %u, the needle set sigma %u", who, ref->sigma, ps->sigma);
        return SPM_E_INVALID;
    }
    if (l->n > 0xFFFFFFFFull) {
        SPM_SET_ERR(ctx, "%s: more than 2^32 - 1 loci", who);
        return SPM_E_UNSUPPORTED;
    }
    SPM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    std::unique_ptr<spm_jst_rescues, void (*)(spm_jst_rescues *)> R(new spm_jst_rescues, spm_hip_jst_rescues_destroy);
    const uint32_t n_pairs = (uint32_t)pr->n;
    R->ctx = ctx;
    R->stats.n_pairs = n_pairs;
    uint32_t n_jobs = 0;
    if (n_pairs) {
        hipStream_t st = ctx->stream;
        hip_events<8> ev;
        SPM_HIP_CHECK(ctx, ev.create());
        SPM_TRY(spm_align_tables(ps)); // the needles' ranks on the device (built once per set)
        jst_rescue_params P{};
        P.loci = l->d_loci;
        P.n = l->d_loci ? (uint32_t)l->n : 0u;
        P.reads = r->d;
        P.pairs = pr->d;
        P.n_pairs = n_pairs;
        P.text = ref->d;
        P.N = ref->n;
        P.sigma = ps->sigma;
        P.ranks = ps->d_al_ranks;
        P.offsets = ps->d_al_offsets;
        P.m = ps->d_m;
        P.min_tlen = opts->min_tlen;
        P.max_tlen = opts->max_tlen;
        P.k = std::min(opts->k, kJstRescueMaxM); // (needles have at most kJstRescueMaxM symbols: the same rule)
        size_t tmp_bytes = 0;
        SPM_HIP_CHECK(ctx, exclusive_sum_tmp_bytes<uint32_t>(ctx, counted<uint32_t>(rescue_cnt_op{nullptr}), n_pairs, &tmp_bytes));
        uint8_t *d_tmp = nullptr;
        scratch_layout L;
        L.take(P.cnt, n_pairs);
        L.take(P.offs, n_pairs);
        L.take(d_tmp, tmp_bytes);
        SPM_TRY(ensure_scratch(ctx, L.bytes()));
        L.bind(ctx->d_scratch);
        dev_scratch keep; // what outlives align_run
        SPM_HIP_CHECK(ctx, keep.alloc(&P.counts, kRescueCnts * 8));
        // ---- the jobs: counted, then written in pair order ----
        SPM_HIP_CHECK(ctx, hipMemsetAsync(P.counts, 0, kRescueCnts * 8, st));
        SPM_HIP_CHECK(ctx, hipEventRecord(ev[0], st));
        SPM_HIP_CHECK(ctx, launch_1d(ctx, jst_rescue_jobs_kernel<false>, n_pairs, P));
        SPM_HIP_CHECK(ctx, hipEventRecord(ev[1], st));
        SPM_HIP_CHECK(ctx, read_counts(ctx, P.counts, kRescueCnts));
        if (ctx->h_counters[kRescueCntBad]) {
            SPM_SET_ERR(ctx, "%s: %llu pair records disagree with the read summary, these loci or the reference; nothing was rescued",
                        who, ctx->h_counters[kRescueCntBad]);
            return SPM_E_INVALID;
        }
        n_jobs = (uint32_t)ctx->h_counters[kRescueCntJobs];
        hipEventElapsedTime(&R->stats.ms_jobs, ev[0], ev[1]);
        if (n_jobs) {
            P.n_jobs = n_jobs;
            SPM_HIP_CHECK(ctx, keep.alloc(&P.jobs, (size_t)n_jobs * sizeof(jst_rescue_job)));
            SPM_HIP_CHECK(ctx, hipMalloc(&R->d, (size_t)n_jobs * sizeof(spm_jst_rescue)));
            R->n = n_jobs;
            SPM_HIP_CHECK(ctx, hipEventRecord(ev[2], st));
            SPM_HIP_CHECK(ctx, exclusive_sum(ctx, d_tmp, tmp_bytes, counted<uint32_t>(rescue_cnt_op{P.cnt}), P.offs, n_pairs));
            SPM_HIP_CHECK(ctx, launch_1d(ctx, jst_rescue_jobs_kernel<true>, n_pairs, P));
            SPM_HIP_CHECK(ctx, hipEventRecord(ev[3], st));
            // ---- the search: one launch per word count the set holds ----
            uint32_t classes = 0;
            for (uint32_t p = 0; p < ps->n; ++p)
                classes |= 1u << (((uint32_t)ps->m[p] + 63) / 64);
            if (classes & 2u)
                SPM_HIP_CHECK(ctx, rescue_search_launch<1>(ctx, P));
            if (classes & 4u)
                SPM_HIP_CHECK(ctx, rescue_search_launch<2>(ctx, P));
            if (classes & 8u)
                SPM_HIP_CHECK(ctx, rescue_search_launch<3>(ctx, P));
            if (classes & 16u)
                SPM_HIP_CHECK(ctx, rescue_search_launch<4>(ctx, P));
            SPM_HIP_CHECK(ctx, hipEventRecord(ev[4], st));
            std::vector<jst_rescue_job> jobs(n_jobs);
            SPM_HIP_CHECK(ctx, hipMemcpyAsync(jobs.data(), P.jobs, (size_t)n_jobs * sizeof(jst_rescue_job), hipMemcpyDeviceToHost, st));
            SPM_HIP_CHECK(ctx, hipStreamSynchronize(st));
            // ---- begins and transcripts of the found jobs: the work list of spm_hip_hits_align ----
            std::vector<spm_hit> hits;
            std::vector<uint64_t> lo;
            std::vector<uint32_t> cig_off, aln_of(n_jobs, kJstPairsNone);
            uint64_t total_ops = 0;
            for (uint32_t j = 0; j < n_jobs; ++j) {
                if (jobs[j].key == kJstRescueNoKey)
                    continue;
                const uint32_t d = jst_rescue_key_d(jobs[j].key);
                aln_of[j] = (uint32_t)hits.size();
                hits.push_back(spm_hit{jobs[j].lo + jst_rescue_key_rel(jobs[j].key), jobs[j].pattern, (int32_t)d});
                lo.push_back(jobs[j].lo);
                cig_off.push_back((uint32_t)total_ops);
                total_ops += 2ull * d + 1;
            }
            if (total_ops > 0xFFFFFFFFull) {
                SPM_SET_ERR(ctx, "%s: the CIGAR pool would exceed 2^32 words", who);
                return SPM_E_UNSUPPORTED;
            }
            spm_align_stats as{};
            uint32_t *d_aln_of = nullptr;
            spm_aln *d_alns = nullptr;
            SPM_HIP_CHECK(ctx, keep.alloc(&d_aln_of, (size_t)n_jobs * 4));
            SPM_HIP_CHECK(ctx, hipMemcpyAsync(d_aln_of, aln_of.data(), (size_t)n_jobs * 4, hipMemcpyHostToDevice, st));
            if (!hits.empty()) {
                R->n_ops = total_ops;
                R->host_ops.resize(total_ops);
                SPM_HIP_CHECK(ctx, hipMalloc(&R->d_ops, total_ops * 4));
                SPM_HIP_CHECK(ctx, keep.alloc(&d_alns, hits.size() * sizeof(spm_aln)));
                align_work W{};
                W.ps = ps;
                W.text = ref;
                W.hits = hits.data();
                W.n = hits.size();
                W.lo = lo.data();
                W.cig_off = cig_off.data();
                W.d_recs = d_alns;
                W.d_ops = R->d_ops;
                W.n_ops = total_ops;
                W.h_ops = R->host_ops.data();
                W.who = who;
                SPM_TRY(align_run(ctx, W, as));
            }
            // ---- the records ----
            P.aln_of = d_aln_of;
            P.alns = d_alns;
            P.n_alns = (uint32_t)hits.size();
            P.out = R->d;
            SPM_HIP_CHECK(ctx, hipEventRecord(ev[5], st));
            SPM_HIP_CHECK(ctx, launch_1d(ctx, jst_rescue_emit_kernel, n_jobs, P));
            SPM_HIP_CHECK(ctx, hipEventRecord(ev[6], st));
            R->host.resize(n_jobs);
            SPM_HIP_CHECK(ctx, hipMemcpyAsync(R->host.data(), R->d, (size_t)n_jobs * sizeof(spm_jst_rescue), hipMemcpyDeviceToHost, st));
            SPM_HIP_CHECK(ctx, read_counts(ctx, P.counts, kRescueCnts)); // (synchronises: the host view has arrived too)
            const unsigned long long *c = ctx->h_counters;
            if (c[kRescueCntBad]) {
                SPM_SET_ERR(ctx, "%s: %llu found jobs without an alignment record", who, c[kRescueCntBad]);
                return SPM_E_INVALID;
            }
            R->stats.n_jobs = n_jobs;
            R->stats.n_rescued = c[kRescueCntRescued];
            R->stats.n_none = c[kRescueCntNone];
            R->stats.n_not_concordant = c[kRescueCntNotConcordant];
            R->stats.n_short = c[kRescueCntShort];
            R->stats.max_window = c[kRescueCntMaxWindow];
            float ms = 0;
            hipEventElapsedTime(&ms, ev[2], ev[3]);
            R->stats.ms_jobs += ms;
            hipEventElapsedTime(&R->stats.ms_search, ev[3], ev[4]);
            R->stats.ms_align = as.ms_total;
            hipEventElapsedTime(&R->stats.ms_emit, ev[5], ev[6]);
        }
        R->stats.ms_total = R->stats.ms_jobs + R->stats.ms_search + R->stats.ms_align + R->stats.ms_emit;
    }
    R->stats.ms_host = ms_since(t_call);
    if (spm_trace_on())
        fprintf(stderr, "[spm_hip] jst rescue: %u pairs -> %u jobs, %llu rescued, %llu none (%llu short), %llu not concordant, longest "
                        "window %llu: device %.3f ms (jobs %.3f, search %.3f, align %.3f, emit %.3f), %.3f ms in all\n", n_pairs, n_jobs,
                (unsigned long long)R->stats.n_rescued, (unsigned long long)R->stats.n_none, (unsigned long long)R->stats.n_short,
                (unsigned long long)R->stats.n_not_concordant, (unsigned long long)R->stats.max_window, R->stats.ms_total,
                R->stats.ms_jobs, R->stats.ms_search, R->stats.ms_align, R->stats.ms_emit, R->stats.ms_host);
    *out = R.release();
    return SPM_OK;
}

extern "C" int spm_hip_jst_rescues_view(spm_jst_rescues *r, const spm_jst_rescue **records, uint64_t *n, const uint32_t **ops,
                                        uint64_t *n_ops)
{
    if (!r)
        return SPM_E_INVALID;
    return pool_out(pool_src<spm_jst_rescue>{r->host.data(), r->n, r->host_ops.data(), r->n_ops}, records, n, ops, n_ops);
}

extern "C" int spm_hip_jst_rescues_device(spm_jst_rescues *r, const void **records, uint64_t *n, const void **ops, uint64_t *n_ops)
{
    if (!r)
        return SPM_E_INVALID;
    return pool_out(pool_src<void, void, void>{r->d, r->n, r->d_ops, r->n_ops}, records, n, ops, n_ops);
}

extern "C" int spm_hip_jst_rescues_stats(const spm_jst_rescues *r, spm_jst_rescues_stats *out)
{
    return r ? r->stats_out(out) : SPM_E_INVALID;
}

// jst_pairs.hpp -- the mates of paired-end reads (spm_hip_jst_ref_loci_pairs; contract in spm_hip.h, scheme in DESIGN.md 4.9,
// the rule in jst_pairs_core.hpp).  gfx950.  Unit: jst_reads.hip.  It reads the loci and the read summary (jst_handles.hpp).  The
// loci of pair p are the contiguous patterns 4p .. 4p + 3, and the read summary holds the bounds of the four
// sub-runs, so pairing is a walk of a window of the other mate's reverse run, found by a lower bound:
//   jst_pairs_best_kernel   one lane per locus.  A lane on a forward locus a walks its partner window, keeps its best partner
//                           in partner[a] and packs (uint32) sum << 32 | a; the segmented scan of wave.hpp (wave_run_scan),
//                           keyed on the pair, leaves every run's minimal key in the run's last lane: one 64-bit atomicMin
//                           per wave and run.  Reverse lanes take part with the empty key.  The longest window goes to
//                           max_window;
//   jst_pairs_count_kernel  the same lanes, the same walk: n_pairs / n_best / n_next against the settled minimum, summed in
//                           64 bits by the same scan: three atomicAdd per wave and run;
//   jst_pairs_emit_kernel   one lane per pair: unpacks the key, reads partner, writes the record and the flags, falls back
//                           to the read summary's primaries, counts each statistic with count_flagged.
// Every record of the read summary is tested against the loci before it is used as an index (jst_pairs_read_ok,
// jst_pairs_covers); what disagrees is counted and fails the call.  Minima and sums do not depend on the order the atomics
// land in: the records are byte-identical across runs.
#pragma once

#include <hip/hip_runtime.h>

#include "internal.hpp"
#include "device_order.hpp"
#include "jst_handles.hpp"
#include "jst_pairs_core.hpp"
#include "scratch_layout.hpp"
#include "wave.hpp"

namespace spm_hip
{

enum {
    kPairsCntBad = 0,
    kPairsCntProper,
    kPairsCntUnique,
    kPairsCntMulti,
    kPairsCntDiscordant,
    kPairsCntOneMate,
    kPairsCntUnmapped,
    kPairsCntMaxWindow,
    kPairsCnts
};
constexpr uint32_t kPairsNoPair = 0xFFFFFFFFu; // (pairs are pattern >> 2: below 2^30)

struct jst_pairs_params
{
    const spm_jst_ref_locus *loci = nullptr;
    uint32_t n = 0;                       // loci
    const spm_jst_read *reads = nullptr;  // [n_reads], n_reads even
    uint32_t n_reads = 0;
    uint32_t min_tlen = 0, max_tlen = 0;
    unsigned long long *minkey = nullptr; // [n_reads / 2] preset to kJstPairsNoKey
    unsigned long long *sums = nullptr;   // [3 * n_reads / 2] preset to zero: n_pairs, n_best, n_next of every pair
    uint32_t *partner = nullptr;          // [n]: written for every forward locus that has a partner
    spm_jst_pair *pairs = nullptr;        // [n_reads / 2]
    unsigned long long *counts = nullptr; // [kPairsCnts]
};

enum { kPairsLaneIdle = 0, kPairsLaneForward, kPairsLaneReverse, kPairsLaneBad };

// What lane i does: its pair, and for a forward locus [lo, hi), the reverse run of the other mate.  Both records the lane
// relies on -- its own read's, the other mate's -- are tested against the loci first.
__device__ __forceinline__ int jpairs_lane(const jst_pairs_params &P, uint32_t i, uint32_t &pair, uint32_t &lo, uint32_t &hi)
{
    const uint32_t pattern = P.loci[i].pattern, read = pattern >> 1;
    if (read >= P.n_reads)
        return kPairsLaneBad;
    if (!jst_pairs_covers(P.reads[read], P.n, i, pattern))
        return kPairsLaneBad;
    pair = jst_pairs_pair(pattern);
    if (jst_pairs_reverse(pattern))
        return kPairsLaneReverse;
    const uint32_t mate = read ^ 1u; // (n_reads is even: below n_reads)
    const spm_jst_read M = P.reads[mate];
    if (!jst_pairs_read_ok(P.loci, P.n, M, mate))
        return kPairsLaneBad;
    lo = M.first_locus + M.n_forward;
    hi = M.first_locus + M.n_loci;
    return kPairsLaneForward;
}

// what jst_pairs_count_kernel carries through the scan over a pair's run, in 64 bits
struct jpairs_count_run
{
    run_sum<unsigned long long> n_pairs, n_best, n_next;
    __device__ __forceinline__ jpairs_count_run up(int d) const { return {n_pairs.up(d), n_best.up(d), n_next.up(d)}; }
    __device__ __forceinline__ void join(const jpairs_count_run &l, bool take)
    {
        n_pairs.join(l.n_pairs, take);
        n_best.join(l.n_best, take);
        n_next.join(l.n_next, take);
    }
};

__global__ __launch_bounds__(256) void jst_pairs_best_kernel(const jst_pairs_params P)
{
    const unsigned long long i = blockIdx.x * 256ull + threadIdx.x;
    uint32_t pair = kPairsNoPair, window = 0;
    unsigned long long key = kJstPairsNoKey, bad = 0;
    if (i < P.n) {
        uint32_t lo = 0, hi = 0;
        const int what = jpairs_lane(P, (uint32_t)i, pair, lo, hi);
        if (what == kPairsLaneBad) {
            pair = kPairsNoPair;
            bad = 1;
        } else if (what == kPairsLaneForward) {
            const jst_pairs_walked W = jst_pairs_walk(P.loci, (uint32_t)i, lo, hi, P.min_tlen, P.max_tlen, -1);
            window = W.window;
            bad = W.unusable;
            if (W.partner != kJstPairsNone) {
                P.partner[i] = W.partner;
                key = jst_pairs_key(W.sum, (uint32_t)i);
            }
        }
    }
    run_min<unsigned long long> R{key};
    const bool ends = wave_run_scan(pair, R);
    if (pair != kPairsNoPair && ends && R.v != kJstPairsNoKey)
        atomicMin(&P.minkey[pair], R.v);
    window = wave_max(window);
    if ((threadIdx.x & 63) == 0 && window)
        atomicMax(&P.counts[kPairsCntMaxWindow], (unsigned long long)window);
    if (bad) // (a fault of the input, not a path to be fast on)
        atomicAdd(&P.counts[kPairsCntBad], bad);
}

__global__ __launch_bounds__(256) void jst_pairs_count_kernel(const jst_pairs_params P)
{
    const unsigned long long i = blockIdx.x * 256ull + threadIdx.x;
    uint32_t pair = kPairsNoPair;
    jpairs_count_run S{{0}, {0}, {0}};
    if (i < P.n) {
        uint32_t lo = 0, hi = 0;
        const int what = jpairs_lane(P, (uint32_t)i, pair, lo, hi);
        if (what == kPairsLaneBad) {
            pair = kPairsNoPair;
        } else if (what == kPairsLaneForward) {
            const unsigned long long key = P.minkey[pair];
            if (key != kJstPairsNoKey) {
                const jst_pairs_walked W = jst_pairs_walk(P.loci, (uint32_t)i, lo, hi, P.min_tlen, P.max_tlen,
                                                          (long long)jst_pairs_key_sum(key));
                S.n_pairs.v = W.n_pairs;
                S.n_best.v = W.n_best;
                S.n_next.v = W.n_next;
            }
        }
    }
    const bool ends = wave_run_scan(pair, S);
    if (pair != kPairsNoPair && ends) {
        if (S.n_pairs.v)
            atomicAdd(&P.sums[3ull * pair], S.n_pairs.v);
        if (S.n_best.v)
            atomicAdd(&P.sums[3ull * pair + 1], S.n_best.v);
        if (S.n_next.v)
            atomicAdd(&P.sums[3ull * pair + 2], S.n_next.v);
    }
}

__global__ __launch_bounds__(256) void jst_pairs_emit_kernel(const jst_pairs_params P)
{
    const unsigned long long p = blockIdx.x * 256ull + threadIdx.x;
    bool bad = false, proper = false, unique = false, multi = false, discordant = false, one_mate = false, unmapped = false;
    if (p < P.n_reads / 2) {
        const spm_jst_read M1 = P.reads[2 * p], M2 = P.reads[2 * p + 1];
        const unsigned long long key = P.minkey[p];
        uint32_t b = kJstPairsNone;
        bad = !jst_pairs_read_ok(P.loci, P.n, M1, (uint32_t)(2 * p)) || !jst_pairs_read_ok(P.loci, P.n, M2, (uint32_t)(2 * p + 1));
        if (!bad && key != kJstPairsNoKey) { // (a: an index a lane of jst_pairs_best_kernel packed, and it wrote partner[a])
            const uint32_t a = jst_pairs_key_a(key);
            bad = a >= P.n || (b = P.partner[a]) >= P.n;
        }
        spm_jst_pair O{};
        if (!bad) {
            O = jst_pairs_record(P.loci, M1.primary, M2.primary, key, b, P.sums[3 * p], P.sums[3 * p + 1], P.sums[3 * p + 2]);
            const bool un1 = (O.flag1 & 0x4u) != 0, un2 = (O.flag1 & 0x8u) != 0;
            proper = (O.flag1 & 0x2u) != 0;
            unique = proper && O.n_best == 1;
            multi = proper && O.n_best > 1;
            discordant = !proper && !un1 && !un2;
            one_mate = un1 != un2;
            unmapped = un1 && un2;
        }
        P.pairs[p] = O;
    }
    count_flagged(&P.counts[kPairsCntBad], bad);
    count_flagged(&P.counts[kPairsCntProper], proper);
    count_flagged(&P.counts[kPairsCntUnique], unique);
    count_flagged(&P.counts[kPairsCntMulti], multi);
    count_flagged(&P.counts[kPairsCntDiscordant], discordant);
    count_flagged(&P.counts[kPairsCntOneMate], one_mate);
    count_flagged(&P.counts[kPairsCntUnmapped], unmapped);
}

} // namespace spm_hip

extern "C" void spm_hip_jst_pairs_destroy(spm_jst_pairs *p) { spm_jst_pairs::destroy(p); }

extern "C" int spm_hip_jst_ref_loci_pairs(spm_jst_ref_loci *l, spm_jst_reads *r, const spm_jst_pair_opts *opts, spm_jst_pairs **out)
{
    using namespace spm_hip;
    if (!l || !out)
        return SPM_E_INVALID;
    spm_ctx *ctx = l->ctx;
    const auto t_call = clk::now();
    if (!r || !opts) {
        SPM_SET_ERR(ctx, "spm_hip_jst_ref_loci_pairs: NULL %s", r ? "opts" : "reads handle");
        return SPM_E_INVALID;
    }
    if (opts->flags || opts->reserved) {
        SPM_SET_ERR(ctx, "spm_hip_jst_ref_loci_pairs: unknown flag bits 0x%x or reserved %u, both must be 0", opts->flags, opts->reserved);
        return SPM_E_INVALID;
    }
    if (!jst_pairs_opts_ok(*opts)) {
        SPM_SET_ERR(ctx, "spm_hip_jst_ref_loci_pairs: min_tlen %u, max_tlen %u: not 1 <= min_tlen <= max_tlen <= 2^31 - 1", opts->min_tlen,
                    opts->max_tlen);
        return SPM_E_INVALID;
    }
    if (r->ctx != ctx) {
        SPM_SET_ERR(ctx, "spm_hip_jst_ref_loci_pairs: the reads handle belongs to another context");
        return SPM_E_INVALID;
    }
    if (r->strands != 2) {
        SPM_SET_ERR(ctx, "spm_hip_jst_ref_loci_pairs: the reads handle was made with strands == %u, mates need a stranded set (2)", r->strands);
        return SPM_E_INVALID;
    }
    if (r->n & 1) {
        SPM_SET_ERR(ctx, "spm_hip_jst_ref_loci_pairs: an odd number of reads (%llu): reads 2p and 2p + 1 are mates", (unsigned long long)r->n);
        return SPM_E_INVALID;
    }
    if (r->n_loci != l->n) {
        SPM_SET_ERR(ctx, "spm_hip_jst_ref_loci_pairs: the reads handle was made from %llu loci, these are %llu", (unsigned long long)r->n_loci,
                    (unsigned long long)l->n);
        return SPM_E_INVALID;
    }
    if (l->n > 0xFFFFFFFFull) {
        SPM_SET_ERR(ctx, "spm_hip_jst_ref_loci_pairs: more than 2^32 - 1 loci");
        return SPM_E_UNSUPPORTED;
    }
    SPM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    std::unique_ptr<spm_jst_pairs, void (*)(spm_jst_pairs *)> R(new spm_jst_pairs, spm_hip_jst_pairs_destroy);
    const uint32_t n_reads = (uint32_t)r->n, n_pairs = n_reads / 2;
    R->ctx = ctx;
    R->n = n_pairs;
    R->stats.n_pairs = n_pairs;
    if (n_pairs) {
        hipStream_t st = ctx->stream;
        hip_events<2> ev;
        SPM_HIP_CHECK(ctx, ev.create());
        jst_pairs_params P{};
        P.loci = l->d_loci;
        P.n = l->d_loci ? (uint32_t)l->n : 0u;
        scratch_layout L;
        L.take(P.minkey, n_pairs);
        L.take(P.sums, 3 * (size_t)n_pairs);
        L.take(P.partner, P.n);
        L.take(P.counts, kPairsCnts);
        SPM_TRY(ensure_scratch(ctx, L.bytes()));
        L.bind(ctx->d_scratch);
        SPM_HIP_CHECK(ctx, hipMalloc(&R->d, (size_t)n_pairs * sizeof(spm_jst_pair)));
        P.reads = r->d;
        P.n_reads = n_reads;
        P.min_tlen = opts->min_tlen;
        P.max_tlen = opts->max_tlen;
        P.pairs = R->d;
        SPM_HIP_CHECK(ctx, hipEventRecord(ev[0], st));
        SPM_HIP_CHECK(ctx, hipMemsetAsync(P.minkey, 0xFF, (size_t)n_pairs * 8, st));
        SPM_HIP_CHECK(ctx, hipMemsetAsync(P.sums, 0, (size_t)n_pairs * 24, st));
        SPM_HIP_CHECK(ctx, hipMemsetAsync(P.counts, 0, kPairsCnts * 8, st));
        if (P.n) {
            SPM_HIP_CHECK(ctx, launch_1d(ctx, jst_pairs_best_kernel, P.n, P));
            SPM_HIP_CHECK(ctx, launch_1d(ctx, jst_pairs_count_kernel, P.n, P));
        }
        SPM_HIP_CHECK(ctx, launch_1d(ctx, jst_pairs_emit_kernel, n_pairs, P));
        SPM_HIP_CHECK(ctx, hipEventRecord(ev[1], st));
        R->host.resize(n_pairs);
        SPM_HIP_CHECK(ctx, hipMemcpyAsync(R->host.data(), R->d, (size_t)n_pairs * sizeof(spm_jst_pair), hipMemcpyDeviceToHost, st));
        SPM_HIP_CHECK(ctx, read_counts(ctx, P.counts, kPairsCnts)); // (synchronises: the host view has arrived too)
        const unsigned long long *c = ctx->h_counters;
        if (c[kPairsCntBad]) {
            SPM_SET_ERR(ctx, "spm_hip_jst_ref_loci_pairs: %llu records of the reads handle disagree with these loci (or score sums "
                             "do not fit in 31 bits); nothing was paired", c[kPairsCntBad]);
            return SPM_E_INVALID;
        }
        R->stats.n_proper = c[kPairsCntProper];
        R->stats.n_unique = c[kPairsCntUnique];
        R->stats.n_multi = c[kPairsCntMulti];
        R->stats.n_discordant = c[kPairsCntDiscordant];
        R->stats.n_one_mate = c[kPairsCntOneMate];
        R->stats.n_unmapped = c[kPairsCntUnmapped];
        R->stats.max_window = c[kPairsCntMaxWindow];
        hipEventElapsedTime(&R->stats.ms_total, ev[0], ev[1]);
    }
    R->stats.ms_host = ms_since(t_call);
    if (spm_trace_on())
        fprintf(stderr, "[spm_hip] jst pairs: %llu loci -> %u pairs, %llu proper (%llu unique, %llu multi), %llu discordant, %llu with "
                        "one mate, %llu unmapped, longest window %llu: device %.3f ms, %.3f ms in all\n", (unsigned long long)l->n,
                n_pairs, (unsigned long long)R->stats.n_proper, (unsigned long long)R->stats.n_unique,
                (unsigned long long)R->stats.n_multi, (unsigned long long)R->stats.n_discordant,
                (unsigned long long)R->stats.n_one_mate, (unsigned long long)R->stats.n_unmapped,
                (unsigned long long)R->stats.max_window, R->stats.ms_total, R->stats.ms_host);
    *out = R.release();
    return SPM_OK;
}

extern "C" int spm_hip_jst_pairs_view(spm_jst_pairs *p, const spm_jst_pair **records, uint64_t *n)
{
    return p ? p->view(records, n) : SPM_E_INVALID;
}

extern "C" int spm_hip_jst_pairs_device(spm_jst_pairs *p, const void **records, uint64_t *n)
{
    return p ? p->device(records, n) : SPM_E_INVALID;
}

extern "C" int spm_hip_jst_pairs_stats(const spm_jst_pairs *p, spm_jst_pairs_stats *out)
{
    return p ? p->stats_out(out) : SPM_E_INVALID;
}

// jst_reads.hpp -- the loci of every read (spm_hip_jst_ref_loci_reads; contract in spm_hip.h, scheme in DESIGN.md 4.8, the
// rule in jst_reads_core.hpp).  gfx950.  Unit: jst_reads.hip.  It reads the collapse's spm_jst_ref_loci (jst_handles.hpp).
// The loci of a collapse are ordered by pattern, so the loci of one read are one contiguous run.  Work is proportional to
// loci + reads, and a read with 10^5 loci is 10^5 lanes, not a loop:
//   jst_reads_min_kernel    one lane per locus: the segmented scan over the wave (wave_run_scan of wave.hpp, here over a
//                           64-bit key and two counts) leaves, in the last lane of every run of one read, the run's
//                           minimal key (uint32) score << 32 | locus and its n_loci / n_forward: one atomicMin and two
//                           atomicAdd per wave and run.  The head of a read's run writes first_locus.  Unusable loci are
//                           counted and index nothing;
//   jst_reads_count_kernel  one lane per locus, the same scan over two counts: n_best / n_next against the settled minimum;
//   jst_reads_emit_kernel   one lane per read: unpacks the key, reads the primary's ref_score, finds where a read without
//                           loci would stand (a lower bound over the patterns), counts mapped / unique / multi reads.
// Minima and counts do not depend on the order the atomics land in: the records are byte-identical across runs.
// The handle is a device_records (device_order.hpp), as are the launches, the events and the read-back.
#pragma once

#include <hip/hip_runtime.h>

#include "internal.hpp"
#include "device_order.hpp"
#include "jst_handles.hpp"
#include "jst_reads_core.hpp"
#include "scratch_layout.hpp"
#include "wave.hpp"

namespace spm_hip
{

enum { kReadsCntBad = 0, kReadsCntMapped, kReadsCntUnique, kReadsCntMulti, kReadsCnts };
constexpr uint32_t kReadsNoRead = 0xFFFFFFFFu; // (reads are < n_reads <= 2^32 - 1)

struct jst_reads_params
{
    const spm_jst_ref_locus *loci = nullptr;
    uint32_t n = 0;                       // loci
    uint32_t strands = 1;
    uint32_t n_reads = 0;
    unsigned long long *minkey = nullptr; // [n_reads] preset to kJstReadsNoKey
    spm_jst_read *reads = nullptr;        // [n_reads] preset to zero
    unsigned long long *counts = nullptr; // [kReadsCnts]
};

// what jst_reads_min_kernel carries through the scan over a read's run: the minimal key, and n_loci / n_forward
struct jreads_min_run
{
    run_min<unsigned long long> key;
    run_sum<uint32_t> n_loci, n_forward;
    __device__ __forceinline__ jreads_min_run up(int d) const { return {key.up(d), n_loci.up(d), n_forward.up(d)}; }
    __device__ __forceinline__ void join(const jreads_min_run &l, bool take)
    {
        key.join(l.key, take);
        n_loci.join(l.n_loci, take);
        n_forward.join(l.n_forward, take);
    }
};

// ... and jst_reads_count_kernel: n_best / n_next
struct jreads_count_run
{
    run_sum<uint32_t> n_best, n_next;
    __device__ __forceinline__ jreads_count_run up(int d) const { return {n_best.up(d), n_next.up(d)}; }
    __device__ __forceinline__ void join(const jreads_count_run &l, bool take)
    {
        n_best.join(l.n_best, take);
        n_next.join(l.n_next, take);
    }
};

// the read of locus i, or kReadsNoRead for an unusable one; score: its score
__device__ __forceinline__ uint32_t jreads_read_of(const jst_reads_params &P, uint32_t i, uint32_t &pattern, int32_t &score)
{
    pattern = P.loci[i].pattern;
    score = P.loci[i].score;
    return jst_reads_usable(pattern, score, P.strands, P.n_reads) ? jst_reads_read(pattern, P.strands) : kReadsNoRead;
}

__global__ __launch_bounds__(256) void jst_reads_min_kernel(const jst_reads_params P)
{
    const unsigned long long i = blockIdx.x * 256ull + threadIdx.x;
    uint32_t read = kReadsNoRead, cnt = 0, fwd = 0;
    unsigned long long key = kJstReadsNoKey;
    bool bad = false;
    if (i < P.n) {
        uint32_t pattern;
        int32_t score;
        read = jreads_read_of(P, (uint32_t)i, pattern, score);
        bad = read == kReadsNoRead;
        if (!bad) {
            key = jst_reads_key(score, (uint32_t)i);
            cnt = 1;
            fwd = jst_reads_forward(pattern, P.strands) ? 1u : 0u;
            if (i == 0 || jst_reads_read(P.loci[i - 1].pattern, P.strands) != read)
                P.reads[read].first_locus = (uint32_t)i;
        }
    }
    jreads_min_run R{{key}, {cnt}, {fwd}};
    const bool ends = wave_run_scan(read, R);
    if (read != kReadsNoRead && ends) {
        atomicMin(&P.minkey[read], R.key.v);
        atomicAdd(&P.reads[read].n_loci, R.n_loci.v);
        if (R.n_forward.v)
            atomicAdd(&P.reads[read].n_forward, R.n_forward.v);
    }
    count_flagged(&P.counts[kReadsCntBad], bad);
}

__global__ __launch_bounds__(256) void jst_reads_count_kernel(const jst_reads_params P)
{
    const unsigned long long i = blockIdx.x * 256ull + threadIdx.x;
    uint32_t read = kReadsNoRead, is_best = 0, is_next = 0;
    if (i < P.n) {
        uint32_t pattern;
        int32_t score;
        read = jreads_read_of(P, (uint32_t)i, pattern, score);
        if (read != kReadsNoRead) {
            const int c = jst_reads_class(score, jst_reads_key_score(P.minkey[read]));
            is_best = c == 0;
            is_next = c == 1;
        }
    }
    jreads_count_run R{{is_best}, {is_next}};
    const bool ends = wave_run_scan(read, R);
    if (read != kReadsNoRead && ends) {
        if (R.n_best.v)
            atomicAdd(&P.reads[read].n_best, R.n_best.v);
        if (R.n_next.v)
            atomicAdd(&P.reads[read].n_next, R.n_next.v);
    }
}

__global__ __launch_bounds__(256) void jst_reads_emit_kernel(const jst_reads_params P)
{
    const unsigned long long r = blockIdx.x * 256ull + threadIdx.x;
    bool mapped = false, unique = false, multi = false;
    if (r < P.n_reads) {
        const unsigned long long key = P.minkey[r];
        spm_jst_read R = P.reads[r];
        if (key == kJstReadsNoKey) {
            // where the read would stand: the first locus whose pattern is not below strands * r
            const unsigned long long first_pat = (unsigned long long)P.strands * r;
            uint32_t lo = 0, hi = P.n;
            while (lo < hi) {
                const uint32_t mid = lo + (hi - lo) / 2;
                if (P.loci[mid].pattern < first_pat)
                    lo = mid + 1;
                else
                    hi = mid;
            }
            R = jst_reads_unmapped(lo);
        } else {
            R.primary = jst_reads_key_locus(key); // (an index a lane of jst_reads_min_kernel packed: below n)
            R.best = jst_reads_key_score(key);
            R.best_ref_score = R.primary < P.n ? P.loci[R.primary].ref_score : -1;
            mapped = true;
            unique = R.n_best == 1;
            multi = R.n_best > 1;
        }
        P.reads[r] = R;
    }
    count_flagged(&P.counts[kReadsCntMapped], mapped);
    count_flagged(&P.counts[kReadsCntUnique], unique);
    count_flagged(&P.counts[kReadsCntMulti], multi);
}

} // namespace spm_hip

extern "C" void spm_hip_jst_reads_destroy(spm_jst_reads *r) { spm_jst_reads::destroy(r); }

extern "C" int spm_hip_jst_ref_loci_reads(spm_jst_ref_loci *l, uint32_t strands, uint32_t n_reads, uint32_t flags,
                                          spm_jst_reads **out)
{
    using namespace spm_hip;
    if (!l || !out)
        return SPM_E_INVALID;
    spm_ctx *ctx = l->ctx;
    const auto t_call = clk::now();
    if (flags) {
        SPM_SET_ERR(ctx, "spm_hip_jst_ref_loci_reads: unknown flag bits 0x%x", flags);
        return SPM_E_INVALID;
    }
    if (strands != 1 && strands != 2) {
        SPM_SET_ERR(ctx, "spm_hip_jst_ref_loci_reads: strands is %u, not 1 or 2", strands);
        return SPM_E_INVALID;
    }
    if ((uint64_t)strands * n_reads > 0xFFFFFFFFull) {
        SPM_SET_ERR(ctx, "spm_hip_jst_ref_loci_reads: %u reads on %u strands do not fit a 32-bit pattern index", n_reads, strands);
        return SPM_E_INVALID;
    }
    if (l->n > 0xFFFFFFFFull) {
        SPM_SET_ERR(ctx, "spm_hip_jst_ref_loci_reads: more than 2^32 - 1 loci");
        return SPM_E_UNSUPPORTED;
    }
    SPM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    std::unique_ptr<spm_jst_reads, void (*)(spm_jst_reads *)> R(new spm_jst_reads, spm_hip_jst_reads_destroy);
    R->ctx = ctx;
    R->n = n_reads;
    R->strands = strands;
    R->n_loci = l->n;
    R->stats.n_reads = n_reads;
    R->stats.n_loci = l->n;
    if (n_reads) {
        hipStream_t st = ctx->stream;
        hip_events<2> ev;
        SPM_HIP_CHECK(ctx, ev.create());
        jst_reads_params P{};
        scratch_layout L;
        L.take(P.minkey, n_reads);
        L.take(P.counts, kReadsCnts);
        SPM_TRY(ensure_scratch(ctx, L.bytes()));
        L.bind(ctx->d_scratch);
        SPM_HIP_CHECK(ctx, hipMalloc(&R->d, (size_t)n_reads * sizeof(spm_jst_read)));
        P.loci = l->d_loci;
        P.n = l->d_loci ? (uint32_t)l->n : 0u;
        P.strands = strands;
        P.n_reads = n_reads;
        P.reads = R->d;
        SPM_HIP_CHECK(ctx, hipEventRecord(ev[0], st));
        SPM_HIP_CHECK(ctx, hipMemsetAsync(P.minkey, 0xFF, (size_t)n_reads * 8, st));
        SPM_HIP_CHECK(ctx, hipMemsetAsync(P.reads, 0, (size_t)n_reads * sizeof(spm_jst_read), st));
        SPM_HIP_CHECK(ctx, hipMemsetAsync(P.counts, 0, kReadsCnts * 8, st));
        if (P.n) {
            SPM_HIP_CHECK(ctx, launch_1d(ctx, jst_reads_min_kernel, P.n, P));
            SPM_HIP_CHECK(ctx, launch_1d(ctx, jst_reads_count_kernel, P.n, P));
        }
        SPM_HIP_CHECK(ctx, launch_1d(ctx, jst_reads_emit_kernel, n_reads, P));
        SPM_HIP_CHECK(ctx, hipEventRecord(ev[1], st));
        R->host.resize(n_reads);
        SPM_HIP_CHECK(ctx, hipMemcpyAsync(R->host.data(), R->d, (size_t)n_reads * sizeof(spm_jst_read), hipMemcpyDeviceToHost, st));
        SPM_HIP_CHECK(ctx, read_counts(ctx, P.counts, kReadsCnts)); // (synchronises: the host view has arrived too)
        const unsigned long long *c = ctx->h_counters;
        if (c[kReadsCntBad]) {
            SPM_SET_ERR(ctx, "spm_hip_jst_ref_loci_reads: %llu loci name a pattern outside %u reads on %u strand(s), or have a "
                             "negative score; nothing was summarised", c[kReadsCntBad], n_reads, strands);
            return SPM_E_INVALID;
        }
        R->stats.n_mapped = c[kReadsCntMapped];
        R->stats.n_unique = c[kReadsCntUnique];
        R->stats.n_multi = c[kReadsCntMulti];
        hipEventElapsedTime(&R->stats.ms_total, ev[0], ev[1]);
    }
    R->stats.ms_host = ms_since(t_call);
    if (spm_trace_on())
        fprintf(stderr, "[spm_hip] jst reads: %llu loci -> %u reads on %u strand(s), %llu mapped (%llu unique, %llu multi): "
                        "device %.3f ms, %.3f ms in all\n", (unsigned long long)l->n, n_reads, strands,
                (unsigned long long)R->stats.n_mapped, (unsigned long long)R->stats.n_unique,
                (unsigned long long)R->stats.n_multi, R->stats.ms_total, R->stats.ms_host);
    *out = R.release();
    return SPM_OK;
}

extern "C" int spm_hip_jst_reads_view(spm_jst_reads *r, const spm_jst_read **records, uint64_t *n)
{
    return r ? r->view(records, n) : SPM_E_INVALID;
}

extern "C" int spm_hip_jst_reads_device(spm_jst_reads *r, const void **records, uint64_t *n)
{
    return r ? r->device(records, n) : SPM_E_INVALID;
}

extern "C" int spm_hip_jst_reads_stats(const spm_jst_reads *r, spm_jst_reads_stats *out)
{
    return r ? r->stats_out(out) : SPM_E_INVALID;
}

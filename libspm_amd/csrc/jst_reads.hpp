// jst_reads.hpp -- the loci of every read (spm_hip_jst_ref_loci_reads; contract in spm_hip.h, scheme in DESIGN.md 4.8, the
// rule in jst_reads_core.hpp).  gfx950.  Included by jst.hip behind jst_collapse.hpp, whose spm_jst_ref_loci it reads.
// The loci of a collapse are ordered by pattern, so the loci of one read are one contiguous run.  Work is proportional to
// loci + reads, and a read with 10^5 loci is 10^5 lanes, not a loop:
//   jst_reads_min_kernel    one lane per locus: a segmented scan over the wave (the sel_run_min idiom of select_walk.hpp, here
//                           over a 64-bit key and two counts) leaves, in the last lane of every run of one read, the run's
//                           minimal key (uint32) score << 32 | locus and its n_loci / n_forward: one atomicMin and two
//                           atomicAdd per wave and run.  The head of a read's run writes first_locus.  Unusable loci are
//                           counted and index nothing;
//   jst_reads_count_kernel  one lane per locus, the same scan: n_best / n_next against the settled minimum;
//   jst_reads_emit_kernel   one lane per read: unpacks the key, reads the primary's ref_score, finds where a read without
//                           loci would stand (a lower bound over the patterns), counts mapped / unique / multi reads.
// Minima and counts do not depend on the order the atomics land in: the records are byte-identical across runs.
#pragma once

#include <hip/hip_runtime.h>

#include "common.hpp"
#include "device_order.hpp"
#include "jst_reads_core.hpp"
#include "scratch_layout.hpp"

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

struct jreads_run
{
    unsigned long long key;
    uint32_t a, b;
    bool ends;
};

// Lanes of one read are contiguous.  Inclusive segmented scan over the wave: the last lane of every run of equal `read`
// (ends) holds the run's minimal key and the sums of a and b.  All lanes call.
__device__ __forceinline__ jreads_run jreads_run_scan(uint32_t read, unsigned long long key, uint32_t a, uint32_t b)
{
    const uint32_t lane = threadIdx.x & 63;
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long k2 = __shfl_up(key, d);
        const uint32_t a2 = __shfl_up(a, d), b2 = __shfl_up(b, d), r2 = __shfl_up(read, d);
        if (lane >= (uint32_t)d && r2 == read) {
            key = k2 < key ? k2 : key;
            a += a2;
            b += b2;
        }
    }
    const uint32_t r_next = __shfl_down(read, 1);
    return jreads_run{key, a, b, lane == 63 || r_next != read};
}

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
    const jreads_run R = jreads_run_scan(read, key, cnt, fwd);
    if (read != kReadsNoRead && R.ends) {
        atomicMin(&P.minkey[read], R.key);
        atomicAdd(&P.reads[read].n_loci, R.a);
        if (R.b)
            atomicAdd(&P.reads[read].n_forward, R.b);
    }
    const unsigned long long bad_mask = __ballot(bad);
    if ((threadIdx.x & 63) == 0 && bad_mask)
        atomicAdd(&P.counts[kReadsCntBad], (unsigned long long)__popcll(bad_mask));
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
    const jreads_run R = jreads_run_scan(read, 0ull, is_best, is_next);
    if (read != kReadsNoRead && R.ends) {
        if (R.a)
            atomicAdd(&P.reads[read].n_best, R.a);
        if (R.b)
            atomicAdd(&P.reads[read].n_next, R.b);
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
    const unsigned long long m0 = __ballot(mapped), m1 = __ballot(unique), m2 = __ballot(multi);
    if ((threadIdx.x & 63) == 0) {
        if (m0)
            atomicAdd(&P.counts[kReadsCntMapped], (unsigned long long)__popcll(m0));
        if (m1)
            atomicAdd(&P.counts[kReadsCntUnique], (unsigned long long)__popcll(m1));
        if (m2)
            atomicAdd(&P.counts[kReadsCntMulti], (unsigned long long)__popcll(m2));
    }
}

} // namespace spm_hip

struct spm_jst_reads
{
    spm_ctx *ctx = nullptr;
    spm_jst_read *d_reads = nullptr;
    uint64_t n = 0;
    uint32_t strands = 1; // what the summary was made with, and from how many loci (spm_hip_jst_ref_loci_pairs asks)
    uint64_t n_loci = 0;
    std::vector<spm_jst_read> host;
    spm_jst_reads_stats stats{};
};
static_assert(sizeof(spm_jst_read) == 32 && sizeof(spm_jst_reads_stats) == 48, "spm_hip.h states these sizes");

extern "C" void spm_hip_jst_reads_destroy(spm_jst_reads *r)
{
    if (!r)
        return;
    if (r->ctx && r->d_reads)
        hipStreamSynchronize(r->ctx->stream);
    hipFree(r->d_reads);
    delete r;
}

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
        scratch_layout L;
        const size_t o_min = L.take((size_t)n_reads * 8), o_counts = L.take(kReadsCnts * 8);
        SPM_TRY(ensure_scratch(ctx, L.bytes()));
        void *base = ctx->d_scratch;
        SPM_HIP_CHECK(ctx, hipMalloc(&R->d_reads, (size_t)n_reads * sizeof(spm_jst_read)));
        jst_reads_params P{};
        P.loci = l->d_loci;
        P.n = l->d_loci ? (uint32_t)l->n : 0u;
        P.strands = strands;
        P.n_reads = n_reads;
        P.minkey = L.at<unsigned long long>(base, o_min);
        P.reads = R->d_reads;
        P.counts = L.at<unsigned long long>(base, o_counts);
        SPM_HIP_CHECK(ctx, hipEventRecord(ev[0], st));
        SPM_HIP_CHECK(ctx, hipMemsetAsync(P.minkey, 0xFF, (size_t)n_reads * 8, st));
        SPM_HIP_CHECK(ctx, hipMemsetAsync(P.reads, 0, (size_t)n_reads * sizeof(spm_jst_read), st));
        SPM_HIP_CHECK(ctx, hipMemsetAsync(P.counts, 0, kReadsCnts * 8, st));
        if (P.n) {
            const unsigned g_loci = (unsigned)(((uint64_t)P.n + 255) / 256);
            hipLaunchKernelGGL(jst_reads_min_kernel, dim3(g_loci), dim3(256), 0, st, P);
            SPM_HIP_CHECK(ctx, hipGetLastError());
            hipLaunchKernelGGL(jst_reads_count_kernel, dim3(g_loci), dim3(256), 0, st, P);
            SPM_HIP_CHECK(ctx, hipGetLastError());
        }
        hipLaunchKernelGGL(jst_reads_emit_kernel, dim3((unsigned)(((uint64_t)n_reads + 255) / 256)), dim3(256), 0, st, P);
        SPM_HIP_CHECK(ctx, hipGetLastError());
        SPM_HIP_CHECK(ctx, hipEventRecord(ev[1], st));
        R->host.resize(n_reads);
        SPM_HIP_CHECK(ctx, hipMemcpyAsync(R->host.data(), R->d_reads, (size_t)n_reads * sizeof(spm_jst_read), hipMemcpyDeviceToHost, st));
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
    if (!r || !records || !n)
        return SPM_E_INVALID;
    *records = r->host.data();
    *n = r->n;
    return SPM_OK;
}

extern "C" int spm_hip_jst_reads_device(spm_jst_reads *r, const void **records, uint64_t *n)
{
    if (!r || !records || !n)
        return SPM_E_INVALID;
    *records = r->d_reads;
    *n = r->n;
    return SPM_OK;
}

extern "C" int spm_hip_jst_reads_stats(const spm_jst_reads *r, spm_jst_reads_stats *out)
{
    if (!r || !out)
        return SPM_E_INVALID;
    *out = r->stats;
    return SPM_OK;
}

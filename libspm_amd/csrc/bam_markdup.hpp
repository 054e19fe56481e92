// bam_markdup.hpp -- duplicate reads and pairs of a BAM handle marked with FLAG 0x400 (spm_hip_bam_markdup,
// spm_hip_bam_markdup_records, spm_hip_bam_markdup_host; contract and rule in spm_hip.h, scheme in DESIGN.md 4.12d, the rule's
// functions in bam_markdup_core.hpp).  gfx950.  Unit: bam_index.hip.  It reads the handles of output_handles.hpp.
//   md_primary_kernel   one lane per line: the record read and tested, primary_of[read] claimed; a second claim is counted;
//   md_ends_kernel      one wave per line, four per workgroup: of a placed primary record the CIGAR's span (lane per item) and
//                       the score of its quality bytes -- dwords loaded on 4-byte borders of the address, whatever the record's
//                       alignment, a byte-wise compare, one wave sum -- into the read's word.  The only stage that touches the
//                       bulk of the stream;
//   md_items_kernel     one lane per item (pairs, then ends): its inverted score, for the first sort;
//   md_keys_kernel      one lane per place of that order: the item's key, for the second, stable sort;
//   md_mark_kernel      one lane per place of the final order: "my key is my left neighbour's" -> dup by read;
//   md_lines_kernel     one lane per line: dup by line, the count;
//   md_write_kernel     one lane per line: the one byte of the copied stream that holds the bit, the line record.
// Vector stores only; the only atomics go to primary_of and to the counters.  No LDS.
#pragma once

#include <hip/hip_runtime.h>

#include "internal.hpp"
#include "bam_index.hpp" // bam_src_dword
#include "bam_markdup_core.hpp"
#include "device_order.hpp"
#include "output_handles.hpp"
#include "wave.hpp"

namespace spm_hip
{

enum { kMdCntBad, kMdCntPairs, kMdCntFragments, kMdCntDupPairs, kMdCntDupFragments, kMdCntDupRecords, kMdCntBeside, kMdCnts };
struct markdup_params
{
    const uint8_t *stream = nullptr;
    uint64_t n_bytes = 0;
    const spm_sam_line *lines = nullptr;
    uint32_t n = 0; // lines, and the most reads there can be
    uint64_t ref_len = 0;
    uint32_t min_qual = 0, pos_bits = 0;
    uint32_t *primary_of = nullptr;     // [n] by read: the line of its primary record, kMdNoLine
    unsigned long long *info = nullptr; // [n] by read: md_info_pack, 0 where the read is not placed
    unsigned long long *key_a = nullptr, *key_b = nullptr; // [n] the sorts' keys, in and out
    uint32_t *idx_a = nullptr, *idx_b = nullptr;           // [n] ... and items
    uint8_t *dup_read = nullptr; // [n] by read
    uint8_t *dup = nullptr;      // [n] by line: the result, in scratch until the call is known to succeed
    unsigned long long *counts = nullptr;
    // the handle form: the copied stream and the new line records
    uint8_t *dst = nullptr;
    spm_sam_line *to = nullptr;
};

__global__ __launch_bounds__(256) void md_primary_kernel(const markdup_params P)
{
    const uint64_t i = blockIdx.x * 256ull + threadIdx.x;
    bool bad = false;
    if (i < P.n) {
        const spm_sam_line L = P.lines[i];
        md_rec M;
        bad = !md_rec_read(P.stream, P.n_bytes, L.offset, L.len, M) || L.read >= P.n;
        if (!bad && md_is_primary(M.R.flag))
            bad = atomicCAS(&P.primary_of[L.read], kMdNoLine, (uint32_t)i) != kMdNoLine;
    }
    count_flagged(&P.counts[kMdCntBad], bad);
}

__global__ __launch_bounds__(256) void md_ends_kernel(const markdup_params P)
{
    const uint32_t lane = threadIdx.x % kWave;
    const uint64_t i = blockIdx.x * 4ull + threadIdx.x / kWave;
    if (i >= P.n)
        return; // (whole waves: i is uniform across the wave, and no workgroup barrier follows)
    const uint64_t off = uniform_u64(P.lines[i].offset);
    const uint32_t len = __builtin_amdgcn_readfirstlane(P.lines[i].len), read = __builtin_amdgcn_readfirstlane(P.lines[i].read);
    md_rec M;
    if (!md_rec_read(P.stream, P.n_bytes, off, len, M) || read >= P.n)
        return; // (counted by md_primary_kernel)
    if (!md_is_primary(M.R.flag) || (M.R.flag & 0x4u) || P.primary_of[read] != (uint32_t)i)
        return;
    // ---- the CIGAR: lane l takes the items l, l + 64, ... (name and CIGAR lie inside the record: md_rec_read) ----
    const uint8_t *c = P.stream + off + kBamFixed + M.R.l_read_name;
    uint64_t span = 0;
    bool clipped = false;
    for (uint32_t k = lane; k < M.R.n_cigar_op; k += kWave)
        md_cigar_item(bam_u32(c + 4 * k), span, clipped);
    span = wave_sum(span);
    clipped = __ballot(clipped) != 0;
    uint32_t u = 0, s = 0;
    if (!md_end_of(M.R, span, clipped, P.ref_len, u, s)) {
        if (lane == 0)
            atomicAdd(&P.counts[kMdCntBad], 1ull);
        return;
    }
    // ---- the score: the dwords that cover [q0, q1), from the 4-byte border of the ADDRESS at or below q0 (q0 >= 36); a
    // caller's buffer need not end on a border, so the stream's last dword may be short ----
    const uint64_t q0 = off + M.qual_at, q1 = q0 + M.l_seq; // (q1 <= off + len <= n_bytes: md_rec_read)
    const uint64_t a0 = q0 - ((reinterpret_cast<uint64_t>(P.stream) + q0) & 3u);
    uint64_t sum = 0;
#pragma unroll 1
    for (uint64_t at = a0 + 4ull * lane; at < q1; at += 4ull * kWave)
        sum += md_score_dword(bam_src_dword(P.stream, P.n_bytes, at), at, q0, q1, P.min_qual);
    sum = wave_sum(sum);
    if (lane == 0)
        P.info[read] = md_info_pack(u, s, (M.R.flag & 1u) != 0, md_score_clamp(sum));
}

template <bool Pairs> __global__ __launch_bounds__(256) void md_items_kernel(const markdup_params P)
{
    const uint64_t j = blockIdx.x * 256ull + threadIdx.x, m = md_n_items(Pairs, P.n);
    bool valid = false;
    if (j < m) {
        valid = md_key_valid(Pairs, md_item_key(Pairs, P.info, P.n, j, P.pos_bits), P.pos_bits);
        P.key_a[j] = md_item_inv_score(Pairs, P.info, P.n, j);
        P.idx_a[j] = (uint32_t)j;
    }
    count_flagged(&P.counts[Pairs ? kMdCntPairs : kMdCntFragments], valid && (Pairs || !md_is_pair_end(P.info, P.n, j)));
}

template <bool Pairs> __global__ __launch_bounds__(256) void md_keys_kernel(const markdup_params P)
{
    const uint64_t j = blockIdx.x * 256ull + threadIdx.x, m = md_n_items(Pairs, P.n);
    if (j >= m)
        return;
    const uint32_t item = P.idx_b[j];
    P.key_a[j] = item < m ? md_item_key(Pairs, P.info, P.n, item, P.pos_bits) : md_key_none(Pairs, P.pos_bits);
    P.idx_a[j] = item;
}

// first place of the sorted end keys whose (u, s) is that of `key`
__device__ __forceinline__ uint64_t md_run_head(const unsigned long long *keys, uint64_t m, uint64_t key)
{
    uint64_t lo = 0, hi = m;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (keys[mid] >> 1 < key >> 1)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

template <bool Pairs> __global__ __launch_bounds__(256) void md_mark_kernel(const markdup_params P)
{
    const uint64_t j = blockIdx.x * 256ull + threadIdx.x, m = md_n_items(Pairs, P.n);
    bool dup = false, beside = false;
    if (j < m) {
        const uint64_t key = P.key_b[j];
        const uint32_t item = P.idx_b[j];
        dup = j > 0 && item < m && md_item_is_dup(Pairs, key, P.key_b[j - 1], P.pos_bits);
        if (dup && Pairs) {
            P.dup_read[2ull * item] = 1;
            P.dup_read[2ull * item + 1] = 1; // (a valid pair: 2 item + 1 < n)
        } else if (dup) {
            P.dup_read[item] = 1;
            beside = (P.key_b[md_run_head(P.key_b, m, key)] & 1u) == 0; // the run begins with a pair end
        }
    }
    count_flagged(&P.counts[Pairs ? kMdCntDupPairs : kMdCntDupFragments], dup);
    if (!Pairs)
        count_flagged(&P.counts[kMdCntBeside], beside);
}

__global__ __launch_bounds__(256) void md_lines_kernel(const markdup_params P)
{
    const uint64_t i = blockIdx.x * 256ull + threadIdx.x;
    bool dup = false;
    if (i < P.n) {
        const uint32_t read = P.lines[i].read;
        dup = read < P.n && P.primary_of[read] == (uint32_t)i && P.dup_read[read];
        P.dup[i] = dup;
    }
    count_flagged(&P.counts[kMdCntDupRecords], dup);
}

// Records are at least 36 bytes and do not overlap, so no two lanes share the byte.
__global__ __launch_bounds__(256) void md_write_kernel(const markdup_params P)
{
    const uint64_t i = blockIdx.x * 256ull + threadIdx.x;
    if (i >= P.n)
        return;
    spm_sam_line L = P.lines[i];
    const bool dup = P.dup[i] != 0;
    L.flag = (uint16_t)((L.flag & ~kMdFlagDup) | (dup ? kMdFlagDup : 0u));
    P.to[i] = L;
    if (L.offset <= P.n_bytes && L.len >= kBamFixed && L.len <= P.n_bytes - L.offset) { // (else counted by md_primary_kernel)
        uint8_t *at = P.dst + L.offset + kMdFlagAt;
        *at = (uint8_t)((*at & ~(kMdFlagDup >> 8)) | (dup ? kMdFlagDup >> 8 : 0u));
    }
}

// ---- the stages of one call: scratch, events and parameters live until the read-back ----
struct markdup_run
{
    dev_scratch keep;
    hip_events<6> ev; // before keys, behind keys, sort, mark, write, frame
    markdup_params P;
    clk::time_point t_call = clk::now();
};

// the items of one kind in their final order in key_b / idx_b: by inverted score, then stably by key
template <bool Pairs> static int markdup_sort(spm_ctx *ctx, const markdup_params &P, void *d_tmp, size_t tmp_bytes)
{
    const uint64_t m = md_n_items(Pairs, P.n);
    SPM_HIP_CHECK(ctx, launch_1d(ctx, md_items_kernel<Pairs>, m, P));
    SPM_HIP_CHECK(ctx, sort_pairs(ctx, d_tmp, tmp_bytes, P.key_a, P.key_b, P.idx_a, P.idx_b, m, md_score_bits(Pairs)));
    SPM_HIP_CHECK(ctx, launch_1d(ctx, md_keys_kernel<Pairs>, m, P));
    SPM_HIP_CHECK(ctx, sort_pairs(ctx, d_tmp, tmp_bytes, P.key_a, P.key_b, P.idx_a, P.idx_b, m, md_key_bits(Pairs, P.pos_bits)));
    return SPM_OK;
}

// keys, sort and mark enqueued on the context's stream; the result lands in run.P.dup, scratch of the run's own (a call that
// fails writes nothing of the caller's).  The inputs have passed markdup_check_args; n > 0.
static int markdup_enqueue(spm_ctx *ctx, markdup_run &run, const uint8_t *d_stream, uint64_t n_bytes, const spm_sam_line *d_lines, uint32_t n,
                           uint64_t ref_len, uint32_t min_qual)
{
    hipStream_t st = ctx->stream;
    markdup_params &P = run.P;
    dev_scratch &keep = run.keep;
    P.stream = d_stream;
    P.n_bytes = n_bytes;
    P.lines = d_lines;
    P.n = n;
    P.ref_len = ref_len;
    P.min_qual = min_qual;
    P.pos_bits = bam_pos_bits(ref_len);
    void *d_tmp = nullptr;
    size_t tmp_bytes = 0;
    SPM_HIP_CHECK(ctx, sort_pairs_tmp_bytes(ctx, n, 64, &tmp_bytes));
    SPM_HIP_CHECK(ctx, keep.alloc(&d_tmp, std::max<size_t>(tmp_bytes, 1)));
    SPM_HIP_CHECK(ctx, keep.alloc(&P.primary_of, (size_t)n * 4));
    SPM_HIP_CHECK(ctx, keep.alloc(&P.info, (size_t)n * 8));
    SPM_HIP_CHECK(ctx, keep.alloc(&P.key_a, (size_t)n * 8));
    SPM_HIP_CHECK(ctx, keep.alloc(&P.key_b, (size_t)n * 8));
    SPM_HIP_CHECK(ctx, keep.alloc(&P.idx_a, (size_t)n * 4));
    SPM_HIP_CHECK(ctx, keep.alloc(&P.idx_b, (size_t)n * 4));
    SPM_HIP_CHECK(ctx, keep.alloc(&P.dup_read, (size_t)n));
    SPM_HIP_CHECK(ctx, keep.alloc(&P.dup, (size_t)n));
    SPM_HIP_CHECK(ctx, hipMemsetAsync(P.primary_of, 0xff, (size_t)n * 4, st));
    SPM_HIP_CHECK(ctx, hipMemsetAsync(P.info, 0, (size_t)n * 8, st));
    SPM_HIP_CHECK(ctx, hipMemsetAsync(P.dup_read, 0, (size_t)n, st));
    SPM_HIP_CHECK(ctx, hipEventRecord(run.ev[0], st));
    // ---- keys ----
    SPM_HIP_CHECK(ctx, launch_1d(ctx, md_primary_kernel, n, P));
    hipLaunchKernelGGL(md_ends_kernel, dim3((n + 3) / 4), dim3(256), 0, st, P);
    SPM_HIP_CHECK(ctx, hipGetLastError());
    SPM_HIP_CHECK(ctx, hipEventRecord(run.ev[1], st));
    // ---- sort, then mark: the pairs' order is used up before the ends take the same buffers ----
    SPM_TRY(markdup_sort<true>(ctx, P, d_tmp, tmp_bytes));
    SPM_HIP_CHECK(ctx, launch_1d(ctx, md_mark_kernel<true>, md_n_items(true, n), P));
    SPM_TRY(markdup_sort<false>(ctx, P, d_tmp, tmp_bytes));
    SPM_HIP_CHECK(ctx, hipEventRecord(run.ev[2], st));
    SPM_HIP_CHECK(ctx, launch_1d(ctx, md_mark_kernel<false>, n, P));
    SPM_HIP_CHECK(ctx, launch_1d(ctx, md_lines_kernel, n, P));
    SPM_HIP_CHECK(ctx, hipEventRecord(run.ev[3], st));
    return SPM_OK;
}

// the one read-back: the disagreements and the counts.  The events 4 and 5 have been recorded by the caller; `file`: it wrote
// and framed a stream between them (the raw form did not: its two times are 0, not what two events in a row measure).
static int markdup_finish(const char *who, spm_ctx *ctx, markdup_run &run, bool file, spm_bam_markdup_stats &S)
{
    SPM_HIP_CHECK(ctx, read_counts(ctx, run.P.counts, kMdCnts));
    const unsigned long long *c = ctx->h_counters;
    if (c[kMdCntBad]) {
        SPM_SET_ERR(ctx, "%s: %llu records disagree with their line records or cannot be marked (a line that leaves the stream, a "
                         "block_size that is not len - 4, a name, CIGAR, seq or qual that leaves the record, a read index beyond the "
                         "lines, a second primary record of one read; a placed primary record with a refID other than 0, pos < 0, an "
                         "end beyond ref_len %llu or an S or H item); nothing was written", who, c[kMdCntBad], (unsigned long long)run.P.ref_len);
        return SPM_E_INVALID;
    }
    S = spm_bam_markdup_stats{};
    hipEventElapsedTime(&S.ms_keys, run.ev[0], run.ev[1]);
    hipEventElapsedTime(&S.ms_sort, run.ev[1], run.ev[2]);
    hipEventElapsedTime(&S.ms_mark, run.ev[2], run.ev[3]);
    if (file) {
        hipEventElapsedTime(&S.ms_write, run.ev[3], run.ev[4]);
        hipEventElapsedTime(&S.ms_frame, run.ev[4], run.ev[5]);
    }
    S.ms_total = S.ms_keys + S.ms_sort + S.ms_mark + S.ms_write + S.ms_frame;
    S.ms_host = ms_since(run.t_call);
    S.n_records = run.P.n;
    S.n_pairs = c[kMdCntPairs];
    S.n_fragments = c[kMdCntFragments];
    S.n_dup_pairs = c[kMdCntDupPairs];
    S.n_dup_fragments = c[kMdCntDupFragments];
    S.n_dup_records = c[kMdCntDupRecords];
    S.n_fragments_beside_pairs = c[kMdCntBeside];
    if (spm_trace_on())
        fprintf(stderr, "[spm_hip] bam markdup: %u records, %llu pairs (%llu duplicates), %llu fragments (%llu duplicates, %llu beside "
                        "pairs): device %.3f ms (keys %.3f, sort %.3f, mark %.3f, write %.3f, frame %.3f), %.3f ms in all\n", run.P.n,
                c[kMdCntPairs], c[kMdCntDupPairs], c[kMdCntFragments], c[kMdCntDupFragments], c[kMdCntBeside], S.ms_total, S.ms_keys,
                S.ms_sort, S.ms_mark, S.ms_write, S.ms_frame, S.ms_host);
    return SPM_OK;
}

// the counters allocated and cleared, the events made
static int markdup_open(spm_ctx *ctx, markdup_run &run)
{
    SPM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    SPM_HIP_CHECK(ctx, run.ev.create());
    SPM_HIP_CHECK(ctx, run.keep.alloc(&run.P.counts, kMdCnts * 8));
    SPM_HIP_CHECK(ctx, hipMemsetAsync(run.P.counts, 0, kMdCnts * 8, ctx->stream));
    return SPM_OK;
}

// what all three forms refuse before anything is read; min_qual: what the opts ask for
static int markdup_check_args(const char *who, spm_ctx *ctx, const void *records, uint64_t n_bytes, const void *lines, uint64_t n_lines,
                              uint64_t ref_len, const spm_bam_markdup_opts *opts, uint32_t &min_qual)
{
    const char *why = (!records && n_bytes)                ? "NULL records with n_record_bytes > 0"
                      : (!lines && n_lines)                ? "NULL lines with n_lines > 0"
                      : (n_lines == 0) != (n_bytes == 0)   ? "records without lines, or lines without records"
                      : (opts && opts->flags)              ? "flags must be 0"
                      : (opts && opts->reserved)           ? "reserved must be 0"
                      : (opts && opts->min_qual > kMdMaxQual) ? "min_qual above 93"
                                                           : nullptr;
    if (why) {
        SPM_SET_ERR(ctx, "%s: %s", who, why);
        return SPM_E_INVALID;
    }
    if (n_lines > 0xFFFFFFFFull) {
        SPM_SET_ERR(ctx, "%s: %llu records are more than 2^32 - 1 (not supported)", who, (unsigned long long)n_lines);
        return SPM_E_UNSUPPORTED;
    }
    if (ref_len >= kMdMaxRefLen) {
        SPM_SET_ERR(ctx, "%s: ref_len %llu is not below 2^30: a pair's key does not fit the sort (not supported)", who,
                    (unsigned long long)ref_len);
        return SPM_E_UNSUPPORTED;
    }
    min_qual = md_min_qual(opts ? opts->min_qual : 0);
    return SPM_OK;
}

} // namespace spm_hip

extern "C" int spm_hip_bam_markdup(spm_bam *b, const spm_bam_markdup_opts *opts, spm_bam **out)
{
    static const char *const who = "spm_hip_bam_markdup";
    if (out)
        *out = nullptr;
    if (!b || !out)
        return SPM_E_INVALID;
    spm_ctx *ctx = b->ctx;
    uint32_t min_qual = 0;
    SPM_TRY(markdup_check_args(who, ctx, b->d_records, b->n_record_bytes, b->d_lines, b->n_lines, b->ref_len, opts, min_qual));
    const uint32_t n = (uint32_t)b->n_lines;
    const uint64_t n_bytes = b->n_record_bytes;
    markdup_run run;
    bam_file file;
    bam_ptr R(nullptr, spm_hip_bam_destroy);
    SPM_TRY(file.open(who, ctx, b->rname.c_str(), b->ref_len, b->block_data, b->sorted, R));
    SPM_TRY(file.place(R.get(), n, n_bytes));
    R->stats = b->stats; // the counts are the source's; the times are this call's
    R->stats.ms_lines = R->stats.ms_measure = R->stats.ms_write = R->stats.ms_stats = 0;
    R->sort_stats = b->sort_stats;
    hipStream_t st = ctx->stream;
    SPM_TRY(markdup_open(ctx, run));
    if (n) {
        SPM_HIP_CHECK(ctx, hipMalloc(&R->d_records, n_bytes));
        SPM_HIP_CHECK(ctx, hipMalloc(&R->d_lines, (size_t)n * sizeof(spm_sam_line)));
        SPM_TRY(markdup_enqueue(ctx, run, b->d_records, n_bytes, b->d_lines, n, b->ref_len, min_qual));
        // ---- write: the stream copied, then one byte per record ----
        run.P.dst = R->d_records;
        run.P.to = R->d_lines;
        SPM_HIP_CHECK(ctx, hipMemcpyAsync(R->d_records, b->d_records, n_bytes, hipMemcpyDeviceToDevice, st));
        SPM_HIP_CHECK(ctx, launch_1d(ctx, md_write_kernel, n, run.P));
    } else {
        for (int i = 0; i < 4; ++i)
            SPM_HIP_CHECK(ctx, hipEventRecord(run.ev[i], st));
    }
    SPM_HIP_CHECK(ctx, hipEventRecord(run.ev[4], st));
    // ---- frame ----
    SPM_TRY(file.frame(R.get()));
    SPM_HIP_CHECK(ctx, hipEventRecord(run.ev[5], st));
    spm_bam_markdup_stats &S = R->markdup_stats;
    SPM_TRY(markdup_finish(who, ctx, run, true, S));
    R->marked = true;
    R->stats.ms_frame = S.ms_frame;
    R->stats.ms_total = S.ms_total;
    R->stats.ms_host = S.ms_host;
    *out = R.release();
    return SPM_OK;
}

extern "C" int spm_hip_bam_markdup_stats(const spm_bam *b, spm_bam_markdup_stats *out)
{
    return stats_out(b && b->marked ? &b->markdup_stats : nullptr, out);
}

extern "C" int spm_hip_bam_markdup_records(spm_ctx *ctx, const void *device_records, uint64_t n_record_bytes, const void *device_lines,
                                           uint64_t n_lines, uint64_t ref_len, const spm_bam_markdup_opts *opts, void *device_dup,
                                           spm_bam_markdup_stats *stats)
{
    static const char *const who = "spm_hip_bam_markdup_records";
    if (!ctx || (!device_dup && n_lines)) {
        SPM_SET_ERR(ctx, "%s: NULL %s", who, !ctx ? "ctx" : "device_dup with n_lines > 0");
        return SPM_E_INVALID;
    }
    uint32_t min_qual = 0;
    SPM_TRY(markdup_check_args(who, ctx, device_records, n_record_bytes, device_lines, n_lines, ref_len, opts, min_qual));
    markdup_run run;
    SPM_TRY(markdup_open(ctx, run));
    hipStream_t st = ctx->stream;
    if (n_lines) {
        SPM_TRY(markdup_enqueue(ctx, run, static_cast<const uint8_t *>(device_records), n_record_bytes,
                                static_cast<const spm_sam_line *>(device_lines), (uint32_t)n_lines, ref_len, min_qual));
    } else {
        for (int i = 0; i < 4; ++i)
            SPM_HIP_CHECK(ctx, hipEventRecord(run.ev[i], st));
    }
    SPM_HIP_CHECK(ctx, hipEventRecord(run.ev[4], st)); // (no write, no frame: both times come out 0)
    SPM_HIP_CHECK(ctx, hipEventRecord(run.ev[5], st));
    spm_bam_markdup_stats S;
    SPM_TRY(markdup_finish(who, ctx, run, false, S));
    if (n_lines) { // (behind the read-back: a call that fails has written nothing)
        SPM_HIP_CHECK(ctx, hipMemcpyAsync(device_dup, run.P.dup, n_lines, hipMemcpyDeviceToDevice, st));
        SPM_HIP_CHECK(ctx, hipStreamSynchronize(st));
    }
    out_if(stats, S);
    return SPM_OK;
}

extern "C" int spm_hip_bam_markdup_host(const void *records, uint64_t n_record_bytes, const spm_sam_line *lines, uint64_t n_lines,
                                        uint64_t ref_len, const spm_bam_markdup_opts *opts, uint8_t *dup)
{
    static const char *const who = "spm_hip_bam_markdup_host";
    if (!dup && n_lines) {
        SPM_SET_ERR((spm_ctx *)nullptr, "%s: NULL dup with n_lines > 0", who);
        return SPM_E_INVALID;
    }
    uint32_t min_qual = 0;
    SPM_TRY(markdup_check_args(who, nullptr, records, n_record_bytes, lines, n_lines, ref_len, opts, min_qual));
    md_counts C;
    if (!markdup_serial(static_cast<const uint8_t *>(records), n_record_bytes, lines, n_lines, ref_len, min_qual, dup, C)) {
        SPM_SET_ERR((spm_ctx *)nullptr, "%s: records that disagree with their line records or cannot be marked", who);
        return SPM_E_INVALID;
    }
    return SPM_OK;
}

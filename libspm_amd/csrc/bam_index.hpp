// bam_index.hpp -- a BAM handle in coordinate order, and the BAI index of a sorted one (spm_hip_bam_sort, spm_hip_bam_index,
// spm_hip_bai_build; contract in spm_hip.h, scheme in DESIGN.md 4.12b, the rule in bam_index_core.hpp).  gfx950.  Unit:
// bam_index.hip.  It reads the handles of output_handles.hpp; of the other units it calls bam_plain_header, bgzf_frame_enqueue and
// bgzf_offsets_ready (internal.hpp).
//   bam_sort_keys_kernel    one lane per record: its key fields out of the stream, the packed key; a record that cannot be read
//                           is counted;
//   bam_sort_place_kernel   one lane per record of the new order: its line record with the new offset;
//   bam_gather_kernel       one wave per record, four per workgroup: len bytes from any source byte to any destination byte.
//                           Lanes load dwords on the source's 4-byte borders, funnel-shift a pair to the destination's
//                           alignment and store whole dwords inside the record; the up to three bytes at either end go as
//                           bytes.  Lane l's upper dword is lane l + 1's lower one and comes by a shuffle; the last lane loads
//                           it.  No store leaves the record's own [offset, offset + len).  No atomics.
//   bai_records_kernel      one lane per record: the item the index takes of it, the order test against the record before it,
//                           the head flag of a run of one bin, atomicMin of its begin into the windows it overlaps (min does
//                           not depend on order), the counts;
//   bai_chunks_kernel       the runs compacted into chunks by the exclusive sum of the head flags;
//   bai_bins_kernel         over the chunks sorted by bin: bin heads, where a bin's run ends, the bytes of every entry;
//   bai_backfill_kernel     one workgroup: the reverse min-scan over the windows;
//   bai_write_bins_kernel, bai_write_rest_kernel   the bytes.
#pragma once

#include <hip/hip_runtime.h>

#include "internal.hpp"
#include "bam_index_core.hpp"
#include "device_order.hpp"
#include "output_handles.hpp"
#include "wave.hpp"

namespace spm_hip
{

enum { kSortCntBad, kSortCntBytes, kSortCnts };
struct bam_sort_params
{
    const uint8_t *src = nullptr; // the record stream; its first byte lies on a 4-byte border (a device allocation)
    uint8_t *dst = nullptr;
    uint64_t n_bytes = 0;
    const spm_sam_line *from = nullptr; // [n] input order
    spm_sam_line *to = nullptr;         // [n] new order
    unsigned long long *key_in = nullptr, *key_out = nullptr;
    uint32_t *idx_in = nullptr, *idx_out = nullptr;
    unsigned long long *off = nullptr; // [n] new offsets
    unsigned long long *counts = nullptr;
    uint32_t n = 0, pos_bits = 0;
};

__global__ __launch_bounds__(256) void bam_sort_keys_kernel(const bam_sort_params P)
{
    const uint64_t i = blockIdx.x * 256ull + threadIdx.x;
    bool bad = false;
    if (i < P.n) {
        bam_rec R;
        bad = !bam_rec_read(P.src, P.n_bytes, P.from[i].offset, P.from[i].len, R);
        const uint64_t key = bad ? 0 : bam_key(R);
        bad = bad || !bam_key_packs(key, P.pos_bits);
        P.key_in[i] = bad ? 0 : bam_key_pack(key, P.pos_bits);
        P.idx_in[i] = (uint32_t)i;
    }
    count_flagged(&P.counts[kSortCntBad], bad);
}

struct bam_sorted_len_op // the length of the record that stands at place j of the new order
{
    const spm_sam_line *from;
    const uint32_t *idx;
    uint32_t n;
    __host__ __device__ uint64_t operator()(uint32_t j) const
    {
        const uint32_t i = idx[j];
        return i < n ? from[i].len : 0;
    }
};

__global__ __launch_bounds__(256) void bam_sort_place_kernel(const bam_sort_params P)
{
    const uint64_t j = blockIdx.x * 256ull + threadIdx.x;
    if (j >= P.n)
        return;
    const uint32_t i = P.idx_out[j];
    spm_sam_line L = P.from[i < P.n ? i : 0];
    L.offset = P.off[j];
    P.to[j] = L;
    if (j + 1 == P.n)
        P.counts[kSortCntBytes] = L.offset + L.len;
}

// the dword at source offset a (src + a on a 4-byte border, a below n_bytes); the last dword of the stream may be short
__device__ __forceinline__ uint32_t bam_src_dword(const uint8_t *src, uint64_t n_bytes, uint64_t a)
{
    if (a + 4 <= n_bytes)
        return *reinterpret_cast<const uint32_t *>(src + a);
    uint32_t v = 0;
    for (uint32_t i = 0; a + i < n_bytes; ++i)
        v |= (uint32_t)src[a + i] << (8 * i);
    return v;
}

// len bytes from src + so to `to`, by one wave; so + len <= n_bytes.  All lanes call it with the same arguments but `lane`.
__device__ __forceinline__ void bam_wave_copy(const uint8_t *src, uint64_t n_bytes, uint64_t so, uint8_t *to, uint32_t len, uint32_t lane)
{
    const uint32_t lead = (0u - (uint32_t)reinterpret_cast<uint64_t>(to)) & 3u;
    const uint32_t e = lead < len ? lead : len; // the bytes in front of the destination's first dword border
    if (lane < e)
        to[lane] = src[so + lane];
    const uint32_t nd = (len - e) / 4, rest = (len - e) & 3u;
    const uint64_t s0 = so + e;
    const uint32_t sh = (uint32_t)s0 & 3u; // destination dword k is bytes sh .. sh + 3 of the source dwords k, k + 1
    const uint64_t a0 = s0 - sh;
    uint32_t *q = reinterpret_cast<uint32_t *>(to + e);
#pragma unroll 1
    for (uint32_t base = 0; base < nd; base += kWave) { // (nd is the same in every lane: the shuffle sees the whole wave)
        const uint32_t k = base + lane;
        const bool on = k < nd;
        const uint32_t lo = on ? bam_src_dword(src, n_bytes, a0 + 4ull * k) : 0u;
        uint32_t hi = __shfl_down(lo, 1);
        if (on && sh && (lane == kWave - 1 || k + 1 == nd))
            hi = bam_src_dword(src, n_bytes, a0 + 4ull * k + 4); // (its first sh bytes are the record's: below so + len)
        if (on)
            q[k] = __builtin_amdgcn_alignbyte(hi, lo, sh);
    }
    if (lane < rest)
        to[e + 4 * nd + lane] = src[s0 + 4ull * nd + lane];
}

__global__ __launch_bounds__(256) void bam_gather_kernel(const bam_sort_params P)
{
    const uint32_t lane = threadIdx.x % kWave;
    const uint64_t j = blockIdx.x * 4ull + threadIdx.x / kWave;
    if (j >= P.n)
        return; // (whole waves: j is uniform across the wave, and no workgroup barrier follows)
    const uint32_t i = P.idx_out[j];
    if (i >= P.n)
        return;
    const uint64_t so = uniform_u64(P.from[i].offset), d0 = uniform_u64(P.to[j].offset);
    const uint32_t len = __builtin_amdgcn_readfirstlane(P.to[j].len);
    // (a line that leaves the stream was counted by the keys stage, lines that overlap show in the total: the host refuses)
    if (so > P.n_bytes || len > P.n_bytes - so || d0 > P.n_bytes || len > P.n_bytes - d0)
        return;
    bam_wave_copy(P.src, P.n_bytes, so, P.dst + d0, len, lane);
}

// ---- the index ----
enum { kBaiCntBad, kBaiCntMapped, kBaiCntUnmapped, kBaiCntNoCoor, kBaiCntMaxEnd, kBaiCntChunks, kBaiCntBins, kBaiCnts };
struct bai_params
{
    const uint8_t *stream = nullptr;
    uint64_t n_bytes = 0;
    const spm_sam_line *lines = nullptr;
    uint32_t n = 0;
    bai_blocks B{};
    unsigned long long *counts = nullptr;
    uint32_t *bin = nullptr;                              // [n] per record: its bin, kBaiNoBin if the index does not bin it
    unsigned long long *begin = nullptr, *end = nullptr;  // [n] per record: virtual offsets
    uint32_t *head = nullptr;                             // [n] 1 where a chunk starts
    unsigned long long *chunk_of = nullptr;               // [n] the exclusive sum of that
    unsigned long long *window = nullptr;                 // [kBaiMaxWindows]
    unsigned long long *ckey_in = nullptr, *ckey_out = nullptr; // [n] the chunks' bins, kBaiNoBin (all ones) behind the last chunk
    uint32_t *cidx_in = nullptr, *cidx_out = nullptr;     // [n] chunk ids
    unsigned long long *c_begin = nullptr, *c_end = nullptr;    // [n] by chunk id
    uint32_t *bin_end = nullptr;                          // [kBaiBins] by bin: where its run of sorted chunks ends
    uint32_t *entry = nullptr;                            // [n] by sorted place: the bytes of the entry
    unsigned long long *entry_off = nullptr;              // [n] the exclusive sum of that
    // known after the read-back
    uint8_t *out = nullptr;
    uint64_t n_placed = 0, n_bins = 0, n_chunks = 0, n_intv = 0, n_mapped = 0, n_unmapped = 0, n_no_coor = 0;
};

__global__ __launch_bounds__(256) void bai_records_kernel(const bai_params P)
{
    const uint64_t i = blockIdx.x * 256ull + threadIdx.x;
    bool bad = false, mapped = false, unmapped = false, no_coor = false, head = false;
    uint32_t ref_end = 0; // (at most 2^29)
    if (i < P.n) {
        bai_item I;
        bool ok = bai_line_follows(P.lines, P.n, P.n_bytes, i) && bai_item_of(P.stream, P.n_bytes, P.B, P.lines[i].offset, P.lines[i].len, I);
        uint32_t bin_before = kBaiNoBin;
        if (ok && i) { // the order test, and the bin the record before this one stands in
            bam_rec R;
            ok = bam_rec_read(P.stream, P.n_bytes, P.lines[i - 1].offset, P.lines[i - 1].len, R) && bam_key(R) <= I.key;
            bin_before = R.ref_id == 0 ? R.bin : kBaiNoBin;
        }
        bad = !ok;
        const bool placed = ok && I.placed;
        P.bin[i] = placed ? I.bin : kBaiNoBin;
        P.begin[i] = I.begin;
        P.end[i] = I.end;
        head = placed && (i == 0 || bin_before != I.bin);
        P.head[i] = head;
        P.cidx_in[i] = (uint32_t)i;
        mapped = placed && !I.unmapped;
        unmapped = placed && I.unmapped;
        no_coor = ok && !I.placed;
        if (placed) {
            ref_end = (uint32_t)I.ref_end;
            for (uint64_t w = I.ref_begin >> kBaiWindowShift; w <= (I.ref_end - 1) >> kBaiWindowShift; ++w)
                atomicMin(&P.window[w], (unsigned long long)I.begin);
        }
    }
    count_flagged(&P.counts[kBaiCntBad], bad);
    count_flagged(&P.counts[kBaiCntMapped], mapped);
    count_flagged(&P.counts[kBaiCntUnmapped], unmapped);
    count_flagged(&P.counts[kBaiCntNoCoor], no_coor);
    count_flagged(&P.counts[kBaiCntChunks], head);
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t other = __shfl_xor(ref_end, o);
        ref_end = other > ref_end ? other : ref_end;
    }
    if ((threadIdx.x & 63) == 0 && ref_end)
        atomicMax(&P.counts[kBaiCntMaxEnd], (unsigned long long)ref_end);
}

struct bai_u32_op
{
    const uint32_t *v;
    __host__ __device__ uint64_t operator()(uint32_t i) const { return v[i]; }
};

__global__ __launch_bounds__(256) void bai_chunks_kernel(const bai_params P)
{
    const uint64_t i = blockIdx.x * 256ull + threadIdx.x;
    if (i >= P.n || P.bin[i] == kBaiNoBin)
        return;
    const uint32_t head = P.head[i], id = (uint32_t)P.chunk_of[i] + head - 1;
    if (id >= P.n)
        return; // (no head in front: the record before this one was counted as bad, and the call fails)
    if (head) {
        P.ckey_in[id] = P.bin[i];
        P.c_begin[id] = P.begin[i];
    }
    if (i + 1 == P.n || P.head[i + 1] || P.bin[i + 1] == kBaiNoBin)
        P.c_end[id] = P.end[i];
}

__global__ __launch_bounds__(256) void bai_bins_kernel(const bai_params P)
{
    const uint64_t j = blockIdx.x * 256ull + threadIdx.x;
    bool head = false;
    if (j < P.n) {
        const uint32_t k = (uint32_t)P.ckey_out[j] & 0xFFFFu;
        const bool valid = k != kBaiNoBin;
        head = valid && (j == 0 || ((uint32_t)P.ckey_out[j - 1] & 0xFFFFu) != k);
        if (valid && (j + 1 == P.n || ((uint32_t)P.ckey_out[j + 1] & 0xFFFFu) != k))
            P.bin_end[k] = (uint32_t)j + 1;
        P.entry[j] = valid ? 16u + (head ? 8u : 0u) : 0u;
    }
    count_flagged(&P.counts[kBaiCntBins], head);
}

// window[w] = min over w' >= w, w < n_intv: lane t owns the windows [t c, (t + 1) c)
__global__ __launch_bounds__(256) void bai_backfill_kernel(const bai_params P)
{
    __shared__ unsigned long long part[256];
    const uint32_t t = threadIdx.x, n = (uint32_t)P.n_intv, c = (n + 255) / 256;
    const uint32_t lo = t * c < n ? t * c : n, hi = lo + c < n ? lo + c : n;
    unsigned long long m = kBaiNoOffset;
    for (uint32_t w = hi; w-- > lo;)
        m = P.window[w] < m ? P.window[w] : m;
    part[t] = m;
    __syncthreads();
    unsigned long long right = kBaiNoOffset; // of the windows behind this lane's
    for (uint32_t u = t + 1; u < 256; ++u)
        right = part[u] < right ? part[u] : right;
    for (uint32_t w = hi; w-- > lo;) {
        right = P.window[w] < right ? P.window[w] : right;
        P.window[w] = right;
    }
}

__device__ __forceinline__ void bai_store32(uint8_t *out, uint64_t at, uint32_t v) { *reinterpret_cast<uint32_t *>(out + at) = v; } // at % 4 == 0
__device__ __forceinline__ void bai_store64(uint8_t *out, uint64_t at, uint64_t v)
{
    bai_store32(out, at, (uint32_t)v);
    bai_store32(out, at + 4, (uint32_t)(v >> 32));
}

__global__ __launch_bounds__(256) void bai_write_bins_kernel(const bai_params P)
{
    const uint64_t j = blockIdx.x * 256ull + threadIdx.x;
    if (j >= P.n_chunks)
        return; // (the chunks stand in front of the sorted places)
    const uint32_t k = (uint32_t)P.ckey_out[j] & 0xFFFFu, id = P.cidx_out[j];
    uint64_t at = 12 + P.entry_off[j];
    if (k >= kBaiBins || id >= P.n || at + P.entry[j] > 12 + 8 * (P.n_bins - (P.n_placed ? 1 : 0)) + 16 * P.n_chunks)
        return; // (cannot be: the counts and the sums come from the same flags)
    if (P.entry[j] == 24) {
        bai_store32(P.out, at, k);
        bai_store32(P.out, at + 4, P.bin_end[k] - (uint32_t)j);
        at += 8;
    }
    bai_store64(P.out, at, P.c_begin[id]);
    bai_store64(P.out, at + 8, P.c_end[id]);
}

// lane w < n_intv: ioffset[w]; lane n_intv: everything else outside the bins
__global__ __launch_bounds__(256) void bai_write_rest_kernel(const bai_params P)
{
    const uint64_t w = blockIdx.x * 256ull + threadIdx.x;
    const bool pseudo = P.n_placed != 0;
    const uint64_t real_bins = P.n_bins - (pseudo ? 1 : 0);
    const uint64_t lin = 12 + 8 * real_bins + 16 * P.n_chunks + (pseudo ? 40 : 0); // where n_intv stands
    if (w < P.n_intv) {
        bai_store64(P.out, lin + 4 + 8 * w, P.window[w]);
    } else if (w == P.n_intv) {
        bai_store32(P.out, 0, 0x01494142u);
        bai_store32(P.out, 4, 1);
        bai_store32(P.out, 8, (uint32_t)P.n_bins);
        if (pseudo) {
            const uint64_t at = lin - 40;
            bai_store32(P.out, at, kBaiPseudoBin);
            bai_store32(P.out, at + 4, 2);
            bai_store64(P.out, at + 8, P.begin[0]);
            bai_store64(P.out, at + 16, P.end[P.n_placed - 1]);
            bai_store64(P.out, at + 24, P.n_mapped);
            bai_store64(P.out, at + 32, P.n_unmapped);
        }
        bai_store32(P.out, lin, (uint32_t)P.n_intv);
        bai_store64(P.out, lin + 4 + 8 * P.n_intv, P.n_no_coor);
    }
}

} // namespace spm_hip

// ---------------------------------------------------------------------------------------------------------------------
// spm_hip_bam_sort
// ---------------------------------------------------------------------------------------------------------------------
extern "C" int spm_hip_bam_sort(spm_bam *b, const spm_bam_sort_opts *opts, spm_bam **out)
{
    static const char *const who = "spm_hip_bam_sort";
    if (out)
        *out = nullptr;
    if (!b || !out)
        return SPM_E_INVALID;
    spm_ctx *ctx = b->ctx;
    const auto t_call = clk::now();
    if (opts && opts->reserved) {
        SPM_SET_ERR(ctx, "%s: reserved is %llu (must be 0)", who, (unsigned long long)opts->reserved);
        return SPM_E_INVALID;
    }
    if (b->n_lines > 0xFFFFFFFFull) {
        SPM_SET_ERR(ctx, "%s: %llu records are more than 2^32 - 1 (not supported)", who, (unsigned long long)b->n_lines);
        return SPM_E_UNSUPPORTED;
    }
    const uint32_t D = b->block_data;
    const uint32_t n = (uint32_t)b->n_lines;
    const uint64_t n_bytes = b->n_record_bytes;
    bam_file file;
    bam_ptr R(nullptr, spm_hip_bam_destroy);
    SPM_TRY(file.open(who, ctx, b->rname.c_str(), b->ref_len, D, true, R));
    SPM_TRY(file.place(R.get(), n, n_bytes));
    R->stats = b->stats; // the counts are the source's; the sizes and times are this file's
    R->stats.ms_lines = R->stats.ms_measure = R->stats.ms_write = R->stats.ms_stats = 0;
    hipStream_t st = ctx->stream;
    hip_events<6> ev;
    SPM_HIP_CHECK(ctx, ev.create());
    dev_scratch keep;
    bam_sort_params P;
    P.n = n;
    P.n_bytes = n_bytes;
    P.pos_bits = bam_pos_bits(b->ref_len);
    const uint32_t key_bits = bam_sort_key_bits(P.pos_bits);
    SPM_HIP_CHECK(ctx, keep.alloc(&P.counts, kSortCnts * 8));
    SPM_HIP_CHECK(ctx, hipMemsetAsync(P.counts, 0, kSortCnts * 8, st));
    SPM_HIP_CHECK(ctx, hipEventRecord(ev[0], st));
    if (n) {
        SPM_HIP_CHECK(ctx, hipMalloc(&R->d_records, std::max<uint64_t>(n_bytes, 1)));
        SPM_HIP_CHECK(ctx, hipMalloc(&R->d_lines, (size_t)n * sizeof(spm_sam_line)));
        P.src = b->d_records;
        P.dst = R->d_records;
        P.from = b->d_lines;
        P.to = R->d_lines;
        void *d_tmp = nullptr, *d_sum_tmp = nullptr;
        size_t tmp_bytes = 0, sum_bytes = 0;
        SPM_HIP_CHECK(ctx, sort_pairs_tmp_bytes(ctx, n, key_bits, &tmp_bytes));
        const auto lens = counted<uint64_t>(bam_sorted_len_op{nullptr, nullptr, 0});
        SPM_HIP_CHECK(ctx, exclusive_sum_tmp_bytes<unsigned long long>(ctx, lens, n, &sum_bytes));
        SPM_HIP_CHECK(ctx, keep.alloc(&d_tmp, std::max<size_t>(tmp_bytes, 1)));
        SPM_HIP_CHECK(ctx, keep.alloc(&d_sum_tmp, std::max<size_t>(sum_bytes, 1)));
        SPM_HIP_CHECK(ctx, keep.alloc(&P.key_in, (size_t)n * 8));
        SPM_HIP_CHECK(ctx, keep.alloc(&P.key_out, (size_t)n * 8));
        SPM_HIP_CHECK(ctx, keep.alloc(&P.idx_in, (size_t)n * 4));
        SPM_HIP_CHECK(ctx, keep.alloc(&P.idx_out, (size_t)n * 4));
        SPM_HIP_CHECK(ctx, keep.alloc(&P.off, (size_t)n * 8));
        // ---- keys ----
        SPM_HIP_CHECK(ctx, launch_1d(ctx, bam_sort_keys_kernel, n, P));
        SPM_HIP_CHECK(ctx, hipEventRecord(ev[1], st));
        // ---- sort ----
        SPM_HIP_CHECK(ctx, sort_pairs(ctx, d_tmp, tmp_bytes, P.key_in, P.key_out, P.idx_in, P.idx_out, n, key_bits));
        SPM_HIP_CHECK(ctx, hipEventRecord(ev[2], st));
        // ---- place ----
        SPM_HIP_CHECK(ctx, exclusive_sum(ctx, d_sum_tmp, sum_bytes, counted<uint64_t>(bam_sorted_len_op{P.from, P.idx_out, n}), P.off, n));
        SPM_HIP_CHECK(ctx, launch_1d(ctx, bam_sort_place_kernel, n, P));
        SPM_HIP_CHECK(ctx, hipEventRecord(ev[3], st));
        // ---- gather ----
        hipLaunchKernelGGL(bam_gather_kernel, dim3((n + 3) / 4), dim3(256), 0, st, P);
        SPM_HIP_CHECK(ctx, hipGetLastError());
    } else {
        for (int i = 1; i < 4; ++i)
            SPM_HIP_CHECK(ctx, hipEventRecord(ev[i], st));
    }
    SPM_HIP_CHECK(ctx, hipEventRecord(ev[4], st));
    // ---- frame ----
    SPM_TRY(file.frame(R.get()));
    SPM_HIP_CHECK(ctx, hipEventRecord(ev[5], st));
    SPM_HIP_CHECK(ctx, read_counts(ctx, P.counts, kSortCnts)); // the one read-back: the error counter and the total
    const unsigned long long *c = ctx->h_counters;
    if (c[kSortCntBad] || c[kSortCntBytes] != n_bytes) {
        SPM_SET_ERR(ctx, "%s: %llu line records do not name a record of the stream with a position inside the reference, or the lines do "
                         "not tile the stream (%llu bytes of %llu); nothing was written", who, c[kSortCntBad], c[kSortCntBytes],
                    (unsigned long long)n_bytes);
        return SPM_E_INVALID;
    }
    spm_bam_sort_stats &S = R->sort_stats;
    hipEventElapsedTime(&S.ms_keys, ev[0], ev[1]);
    hipEventElapsedTime(&S.ms_sort, ev[1], ev[2]);
    hipEventElapsedTime(&S.ms_place, ev[2], ev[3]);
    hipEventElapsedTime(&S.ms_gather, ev[3], ev[4]);
    hipEventElapsedTime(&S.ms_frame, ev[4], ev[5]);
    S.ms_total = S.ms_keys + S.ms_sort + S.ms_place + S.ms_gather + S.ms_frame;
    S.ms_host = ms_since(t_call);
    S.key_bits = key_bits;
    S.n_records = n;
    S.n_record_bytes = n_bytes;
    R->stats.ms_frame = S.ms_frame;
    R->stats.ms_total = S.ms_total;
    R->stats.ms_host = S.ms_host;
    if (spm_trace_on())
        fprintf(stderr, "[spm_hip] bam sort: %u records, %llu bytes, %u key bits: device %.3f ms (keys %.3f, sort %.3f, place %.3f, gather "
                        "%.3f, frame %.3f), %.3f ms in all\n", n, (unsigned long long)n_bytes, key_bits, S.ms_total, S.ms_keys, S.ms_sort,
                S.ms_place, S.ms_gather, S.ms_frame, S.ms_host);
    *out = R.release();
    return SPM_OK;
}

extern "C" int spm_hip_bam_sort_stats(const spm_bam *b, spm_bam_sort_stats *out)
{
    return stats_out(b && b->sorted ? &b->sort_stats : nullptr, out);
}

// ---------------------------------------------------------------------------------------------------------------------
// the index
// ---------------------------------------------------------------------------------------------------------------------
extern "C" void spm_hip_bai_destroy(spm_bai *z)
{
    if (z)
        handle_destroy(z, {z->d});
}

// the stages on the context's stream; B.table is a device pointer or null.  The inputs have passed the host's checks.
static int bai_run(const char *who, spm_ctx *ctx, const uint8_t *d_stream, uint64_t n_bytes, const spm_sam_line *d_lines, uint64_t n_lines,
                   const bai_blocks &B, spm_bai **out)
{
    const auto t_call = clk::now();
    SPM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    std::unique_ptr<spm_bai, void (*)(spm_bai *)> Z(new spm_bai, spm_hip_bai_destroy);
    Z->ctx = ctx;
    hipStream_t st = ctx->stream;
    hip_events<5> ev;
    SPM_HIP_CHECK(ctx, ev.create());
    dev_scratch keep;
    bai_params P;
    P.stream = d_stream;
    P.n_bytes = n_bytes;
    P.lines = d_lines;
    P.n = (uint32_t)n_lines;
    P.B = B;
    const uint32_t n = P.n;
    SPM_HIP_CHECK(ctx, keep.alloc(&P.counts, kBaiCnts * 8));
    SPM_HIP_CHECK(ctx, hipMemsetAsync(P.counts, 0, kBaiCnts * 8, st));
    SPM_HIP_CHECK(ctx, keep.alloc(&P.window, (size_t)kBaiMaxWindows * 8));
    SPM_HIP_CHECK(ctx, hipMemsetAsync(P.window, 0xff, (size_t)kBaiMaxWindows * 8, st));
    SPM_HIP_CHECK(ctx, hipEventRecord(ev[0], st));
    if (n) {
        void *d_tmp = nullptr, *d_sum_tmp = nullptr;
        size_t tmp_bytes = 0, sum_bytes = 0;
        SPM_HIP_CHECK(ctx, sort_pairs_tmp_bytes(ctx, n, 16, &tmp_bytes));
        SPM_HIP_CHECK(ctx, exclusive_sum_tmp_bytes<unsigned long long>(ctx, counted<uint64_t>(bai_u32_op{nullptr}), n, &sum_bytes));
        SPM_HIP_CHECK(ctx, keep.alloc(&d_tmp, std::max<size_t>(tmp_bytes, 1)));
        SPM_HIP_CHECK(ctx, keep.alloc(&d_sum_tmp, std::max<size_t>(sum_bytes, 1)));
        SPM_HIP_CHECK(ctx, keep.alloc(&P.bin, (size_t)n * 4));
        SPM_HIP_CHECK(ctx, keep.alloc(&P.begin, (size_t)n * 8));
        SPM_HIP_CHECK(ctx, keep.alloc(&P.end, (size_t)n * 8));
        SPM_HIP_CHECK(ctx, keep.alloc(&P.head, (size_t)n * 4));
        SPM_HIP_CHECK(ctx, keep.alloc(&P.chunk_of, (size_t)n * 8));
        SPM_HIP_CHECK(ctx, keep.alloc(&P.ckey_in, (size_t)n * 8));
        SPM_HIP_CHECK(ctx, keep.alloc(&P.ckey_out, (size_t)n * 8));
        SPM_HIP_CHECK(ctx, keep.alloc(&P.cidx_in, (size_t)n * 4));
        SPM_HIP_CHECK(ctx, keep.alloc(&P.cidx_out, (size_t)n * 4));
        SPM_HIP_CHECK(ctx, keep.alloc(&P.c_begin, (size_t)n * 8));
        SPM_HIP_CHECK(ctx, keep.alloc(&P.c_end, (size_t)n * 8));
        SPM_HIP_CHECK(ctx, keep.alloc(&P.bin_end, (size_t)kBaiBins * 4));
        SPM_HIP_CHECK(ctx, keep.alloc(&P.entry, (size_t)n * 4));
        SPM_HIP_CHECK(ctx, keep.alloc(&P.entry_off, (size_t)n * 8));
        SPM_HIP_CHECK(ctx, hipMemsetAsync(P.ckey_in, 0xff, (size_t)n * 8, st)); // (kBaiNoBin in the 16 bits the sort reads)
        SPM_HIP_CHECK(ctx, hipMemsetAsync(P.bin_end, 0, (size_t)kBaiBins * 4, st));
        // ---- records ----
        SPM_HIP_CHECK(ctx, launch_1d(ctx, bai_records_kernel, n, P));
        SPM_HIP_CHECK(ctx, hipEventRecord(ev[1], st));
        // ---- chunks: compacted, then ordered by bin (stable: a bin's chunks stay in file order) ----
        SPM_HIP_CHECK(ctx, exclusive_sum(ctx, d_sum_tmp, sum_bytes, counted<uint64_t>(bai_u32_op{P.head}), P.chunk_of, n));
        SPM_HIP_CHECK(ctx, launch_1d(ctx, bai_chunks_kernel, n, P));
        SPM_HIP_CHECK(ctx, sort_pairs(ctx, d_tmp, tmp_bytes, P.ckey_in, P.ckey_out, P.cidx_in, P.cidx_out, n, 16));
        SPM_HIP_CHECK(ctx, hipEventRecord(ev[2], st));
        // ---- bins ----
        SPM_HIP_CHECK(ctx, launch_1d(ctx, bai_bins_kernel, n, P));
        SPM_HIP_CHECK(ctx, exclusive_sum(ctx, d_sum_tmp, sum_bytes, counted<uint64_t>(bai_u32_op{P.entry}), P.entry_off, n));
    } else {
        SPM_HIP_CHECK(ctx, hipEventRecord(ev[1], st));
        SPM_HIP_CHECK(ctx, hipEventRecord(ev[2], st));
    }
    SPM_HIP_CHECK(ctx, hipEventRecord(ev[3], st));
    SPM_HIP_CHECK(ctx, read_counts(ctx, P.counts, kBaiCnts)); // the one read-back: the counts, which give the size, and the errors
    const unsigned long long *c = ctx->h_counters;
    if (c[kBaiCntBad]) {
        SPM_SET_ERR(ctx, "%s: %llu records are out of coordinate order, or their line records, the stream and the block offsets disagree "
                         "(a line that leaves the stream or does not follow the one before it, a block_size that is not len - 4, a CIGAR "
                         "that leaves its record, a refID other than 0 and -1, an end beyond 2^29); nothing was written", who, c[kBaiCntBad]);
        return SPM_E_INVALID;
    }
    P.n_mapped = c[kBaiCntMapped];
    P.n_unmapped = c[kBaiCntUnmapped];
    P.n_no_coor = c[kBaiCntNoCoor];
    P.n_placed = P.n_mapped + P.n_unmapped;
    P.n_chunks = c[kBaiCntChunks];
    P.n_bins = c[kBaiCntBins] + (P.n_placed ? 1 : 0);
    P.n_intv = bai_n_intv(c[kBaiCntMaxEnd]);
    Z->n = bai_size(P.n_bins, P.n_chunks, P.n_intv, P.n_placed != 0);
    SPM_HIP_CHECK(ctx, hipMalloc(&Z->d, Z->n));
    P.out = Z->d;
    // ---- write ----
    if (P.n_intv) {
        hipLaunchKernelGGL(bai_backfill_kernel, dim3(1), dim3(256), 0, st, P);
        SPM_HIP_CHECK(ctx, hipGetLastError());
    }
    if (P.n_chunks)
        SPM_HIP_CHECK(ctx, launch_1d(ctx, bai_write_bins_kernel, P.n_chunks, P));
    SPM_HIP_CHECK(ctx, launch_1d(ctx, bai_write_rest_kernel, P.n_intv + 1, P));
    SPM_HIP_CHECK(ctx, hipEventRecord(ev[4], st));
    SPM_HIP_CHECK(ctx, hipEventSynchronize(ev[4])); // (the inputs are the caller's again, and the scratch goes out of scope)
    spm_bai_stats &S = Z->stats;
    hipEventElapsedTime(&S.ms_records, ev[0], ev[1]);
    hipEventElapsedTime(&S.ms_chunks, ev[1], ev[2]);
    hipEventElapsedTime(&S.ms_bins, ev[2], ev[3]);
    hipEventElapsedTime(&S.ms_write, ev[3], ev[4]);
    S.ms_total = S.ms_records + S.ms_chunks + S.ms_bins + S.ms_write;
    S.ms_host = ms_since(t_call);
    S.n_bins = P.n_bins;
    S.n_chunks = P.n_chunks;
    S.n_intv = P.n_intv;
    S.n_mapped = P.n_mapped;
    S.n_unmapped = P.n_unmapped;
    S.n_no_coor = P.n_no_coor;
    S.n_bytes = Z->n;
    if (spm_trace_on())
        fprintf(stderr, "[spm_hip] bai: %u records -> %llu bins, %llu chunks, %llu windows, %llu bytes: device %.3f ms (records %.3f, chunks "
                        "%.3f, bins %.3f, write %.3f), %.3f ms in all\n", n, (unsigned long long)S.n_bins, (unsigned long long)S.n_chunks,
                (unsigned long long)S.n_intv, (unsigned long long)S.n_bytes, S.ms_total, S.ms_records, S.ms_chunks, S.ms_bins, S.ms_write,
                S.ms_host);
    *out = Z.release();
    return SPM_OK;
}

// what both forms and the host form refuse before anything is read
static int bai_check_args(const char *who, spm_ctx *ctx, const void *records, uint64_t n_bytes, const void *lines, uint64_t n_lines,
                          const void *offsets, uint64_t n_blocks, uint32_t block_data, bool need_offsets)
{
    const char *why = (!records && n_bytes)                              ? "NULL records with n_record_bytes > 0"
                      : (!lines && n_lines)                              ? "NULL lines with n_lines > 0"
                      : (!offsets && need_offsets)                       ? "NULL block_offsets"
                      : block_data > kBgzfBlockData                      ? "block_data above 65280"
                      : (n_lines == 0) != (n_bytes == 0)                 ? "records without lines, or lines without records"
                      : n_blocks != bgzf_n_blocks(n_bytes, bgzf_block_data(block_data)) ? "n_blocks is not what n_record_bytes in blocks of block_data give"
                                                                         : nullptr;
    if (why) {
        SPM_SET_ERR(ctx, "%s: %s", who, why);
        return SPM_E_INVALID;
    }
    if (n_lines > 0xFFFFFFFFull) {
        SPM_SET_ERR(ctx, "%s: %llu records are more than 2^32 - 1 (not supported)", who, (unsigned long long)n_lines);
        return SPM_E_UNSUPPORTED;
    }
    return SPM_OK;
}

extern "C" int spm_hip_bai_build(spm_ctx *ctx, const void *device_records, uint64_t n_record_bytes, const void *device_lines, uint64_t n_lines,
                                 const void *device_block_offsets, uint64_t n_blocks, uint32_t block_data, spm_bai **out)
{
    static const char *const who = "spm_hip_bai_build";
    if (out)
        *out = nullptr;
    if (!ctx || !out) {
        SPM_SET_ERR(ctx, "%s: NULL %s", who, !ctx ? "ctx" : "out");
        return SPM_E_INVALID;
    }
    SPM_TRY(bai_check_args(who, ctx, device_records, n_record_bytes, device_lines, n_lines, device_block_offsets, n_blocks, block_data, true));
    bai_blocks B;
    B.table = static_cast<const unsigned long long *>(device_block_offsets);
    B.n_stream = n_record_bytes;
    B.n_blocks = n_blocks;
    B.D = bgzf_block_data(block_data);
    return bai_run(who, ctx, static_cast<const uint8_t *>(device_records), n_record_bytes, static_cast<const spm_sam_line *>(device_lines),
                   n_lines, B, out);
}

extern "C" int spm_hip_bam_index(spm_bam *b, spm_bgzf *deflated, spm_bai **out)
{
    static const char *const who = "spm_hip_bam_index";
    if (out)
        *out = nullptr;
    if (!b || !out)
        return SPM_E_INVALID;
    spm_ctx *ctx = b->ctx;
    bai_blocks B;
    B.n_stream = b->n_record_bytes;
    B.n_blocks = bgzf_n_blocks(b->n_record_bytes, b->block_data);
    B.D = b->block_data;
    B.first = b->stats.header_file_bytes;
    if (deflated) {
        if (deflated->ctx != ctx || deflated->stats.n_in != b->n_record_bytes || deflated->D != b->block_data ||
            deflated->stats.n_blocks != B.n_blocks) {
            SPM_SET_ERR(ctx, "%s: the deflated file is not this handle's: another context, %llu input bytes in blocks of %u where the "
                             "handle has %llu in blocks of %u", who, (unsigned long long)deflated->stats.n_in, deflated->D,
                        (unsigned long long)b->n_record_bytes, b->block_data);
            return SPM_E_INVALID;
        }
        SPM_TRY(bgzf_offsets_ready(deflated, true));
        B.table = deflated->d_offsets;
    }
    return bai_run(who, ctx, b->d_records, b->n_record_bytes, b->d_lines, b->n_lines, B, out);
}

extern "C" int spm_hip_bai_build_host(const void *records, uint64_t n_record_bytes, const spm_sam_line *lines, uint64_t n_lines,
                                      const uint64_t *block_offsets, uint64_t n_blocks, uint32_t block_data, void *dst, uint64_t cap,
                                      uint64_t *len)
{
    static const char *const who = "spm_hip_bai_build_host";
    if (!len || (!dst && cap)) {
        SPM_SET_ERR((spm_ctx *)nullptr, "%s: NULL %s", who, !len ? "len" : "dst with cap > 0");
        return SPM_E_INVALID;
    }
    SPM_TRY(bai_check_args(who, nullptr, records, n_record_bytes, lines, n_lines, block_offsets, n_blocks, block_data, true));
    bai_blocks B;
    B.table = reinterpret_cast<const unsigned long long *>(block_offsets);
    B.n_stream = n_record_bytes;
    B.n_blocks = n_blocks;
    B.D = bgzf_block_data(block_data);
    std::vector<uint8_t> bytes;
    bai_counts C;
    if (!bai_build_serial(static_cast<const uint8_t *>(records), n_record_bytes, lines, n_lines, B, bytes, C)) {
        SPM_SET_ERR((spm_ctx *)nullptr, "%s: records out of coordinate order, or line records, stream and block offsets that disagree", who);
        return SPM_E_INVALID;
    }
    *len = bytes.size();
    if (bytes.size() > cap)
        return SPM_E_OVERFLOW;
    memcpy(dst, bytes.data(), bytes.size());
    return SPM_OK;
}

extern "C" int spm_hip_bai_view(spm_bai *z, const void **bytes, uint64_t *n)
{
    if (!z)
        return SPM_E_INVALID;
    SPM_TRY(handle_download(z->ctx, z->have_host, view_part{z->d, z->n, z->host}));
    out_if(bytes, z->host.data());
    out_if(n, z->n);
    return SPM_OK;
}

extern "C" int spm_hip_bai_device(spm_bai *z, const void **bytes, uint64_t *n)
{
    if (!z)
        return SPM_E_INVALID;
    out_if(bytes, z->d);
    out_if(n, z->n);
    return SPM_OK;
}

extern "C" int spm_hip_bai_stats(const spm_bai *z, spm_bai_stats *out) { return stats_out(z ? &z->stats : nullptr, out); }

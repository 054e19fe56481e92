// bam_pileup.hpp -- the per-base pileup of a coordinate-sorted BAM handle and the variant sites of a pileup (spm_hip_bam_pileup,
// spm_hip_bam_pileup_records, spm_hip_bam_pileup_host, spm_hip_pileup_sites, spm_hip_pileup_sites_host; contract and rule in
// spm_hip.h, scheme in DESIGN.md 4.12e, the rule's functions in bam_pileup_core.hpp).  gfx950.  Unit: bam_pileup.hip.  It reads
// the handles of output_handles.hpp.
//   pu_records_kernel   one lane per line: the record read and tested, whether it takes part, the order test against its left
//                       neighbour, the disagreements counted; pos[i], and end[i] (0 where the record does not take part);
//   (device_order.hip)  the inclusive running maximum pmax[] of end[]: pmax and pos are monotone, so the records that reach into a
//                       tile [t0, t1) lie between the first i with pmax[i] > t0 and the first with pos[i] >= t1, two binary searches;
//   pu_tiles_kernel     one workgroup per tile of kPuTile positions, its 8 x kPuTile counters in LDS, cleared by the group.  The
//                       four waves draw the candidates in turn; a wave reads the record's CIGAR words (lane per word), then walks
//                       the columns of each item 64 at a time, clipped to tile and region: SEQ nibble and quality byte out of dwords
//                       loaded on 4-byte borders of the address, whatever the record's alignment, one LDS atomic add per column.
//                       Behind a barrier the group stores its eight plane segments, coalesced.  Every counter of the output is
//                       written by exactly one group: no memset, no global atomic on the bulk path;
//   pu_summary_kernel   n_covered, sum_depth, max_depth and the sum of all planes: a block reduction, one atomic per block and value;
//   pu_sites_flag_kernel, (device_order.hip: the exclusive sum), pu_sites_scatter_kernel   the columns that depart from the
//                       reference, compacted in position order.
// Vector stores only; the only global atomics go to the counters.
#pragma once

#include <algorithm>
#include <memory>

#include <hip/hip_runtime.h>

#include "internal.hpp"
#include "bam_pileup_core.hpp"
#include "device_order.hpp"
#include "output_handles.hpp"
#include "wave.hpp"

namespace spm_hip
{

// Positions per tile.  8 planes x 1024 x 4 B = 32 KiB of the CU's 160 KiB of LDS: five groups of four waves per CU hide each
// other's loads, and a read of 100-150 bases reaches into 1.1-1.15 tiles on average.
constexpr uint32_t kPuTile = 1024;
enum { kPuCntBad, kPuCntTaking, kPuCntVisits, kPuCntCovered, kPuCntSumDepth, kPuCntMaxDepth, kPuCntEvidence, kPuCnts };

struct pileup_params
{
    const uint8_t *stream = nullptr;
    uint64_t n_bytes = 0;
    const spm_sam_line *lines = nullptr;
    uint32_t n = 0; // lines
    uint64_t ref_len = 0;
    pu_opts O;
    uint32_t *pos = nullptr, *end = nullptr, *pmax = nullptr; // [n]
    uint32_t *out = nullptr;                                  // [8 * np] plane-major
    uint64_t np = 0;                                          // O.end - O.begin
    unsigned long long *counts = nullptr;
};

__global__ __launch_bounds__(256) void pu_records_kernel(const pileup_params P)
{
    const uint64_t i = blockIdx.x * 256ull + threadIdx.x;
    bool bad = false, takes = false;
    if (i < P.n) {
        const spm_sam_line L = P.lines[i];
        pu_rec R;
        uint64_t end = 0;
        const pu_status s = pu_rec_test(P.stream, P.n_bytes, L.offset, L.len, P.ref_len, P.O, R, end);
        bad = s == kPuBad;
        takes = s == kPuTakes;
        if (!bad && i > 0) {
            const spm_sam_line Lp = P.lines[i - 1];
            bam_rec prev;
            if (bam_rec_read(P.stream, P.n_bytes, Lp.offset, Lp.len, prev)) // (a neighbour that cannot be read is counted by its own lane)
                bad = !pu_order_ok(prev, R.M.R);
        }
        P.pos[i] = bad ? kPuNoPos : pu_pos_key(R.M.R);
        P.end[i] = takes && !bad ? (uint32_t)end : 0u; // (end <= ref_len <= 2^31)
    }
    count_flagged(&P.counts[kPuCntBad], bad);
    count_flagged(&P.counts[kPuCntTaking], takes && !bad);
}

// the dword at stream offset a (stream + a on a 4-byte border, a below n_bytes); a caller's buffer need not end on a border, so the
// stream's last dword may be short (bam_index.hpp's bam_src_dword, which lives in the unit that defines the sort's entry points)
__device__ __forceinline__ uint32_t pu_src_dword(const uint8_t *stream, uint64_t n_bytes, uint64_t a)
{
    if (a + 4 <= n_bytes)
        return *reinterpret_cast<const uint32_t *>(stream + a);
    uint32_t v = 0;
    for (uint32_t i = 0; a + i < n_bytes; ++i)
        v |= (uint32_t)stream[a + i] << (8 * i);
    return v;
}

// One record that takes part (pu_rec_test has passed it: name, CIGAR, SEQ and QUAL lie inside the record, every op is 8 or less,
// the CIGAR's query length is l_seq), walked by one wave and added to the tile's counters.  [lo, hi): the tile cut to the
// region, hi - t0 <= kPuTile.  All lanes call it with the same arguments but `lane`.
__device__ __forceinline__ void pu_wave_walk(const pileup_params &P, uint64_t off, const pu_rec &R, uint64_t t0, uint64_t lo, uint64_t hi,
                                             uint32_t *cnt, uint32_t lane)
{
    const uint8_t *stream = P.stream;
    const uint64_t n_bytes = P.n_bytes;
    const uint32_t mis = (uint32_t)(reinterpret_cast<uint64_t>(stream) & 3u), min_baseq = P.O.min_baseq;
    auto load = [stream, n_bytes](uint64_t a) { return pu_src_dword(stream, n_bytes, a); };
    const uint8_t *c = stream + off + R.cigar_at;
    const uint64_t s0 = off + R.seq_at, q0 = off + R.M.qual_at, pos = (uint64_t)(int64_t)R.M.R.pos;
    const uint32_t n_items = R.M.R.n_cigar_op;
    uint64_t r = pos, q = 0;
#pragma unroll 1
    for (uint32_t base = 0; base < n_items; base += kWave) {
        const uint32_t mine = base + lane < n_items ? bam_u32(c + 4ull * (base + lane)) : 0u;
        const uint32_t m = n_items - base < kWave ? n_items - base : kWave;
#pragma unroll 1
        for (uint32_t k = 0; k < m; ++k) {
            if (r > hi)
                return; // (uniform: nothing behind this item reaches the tile, not even an I at column r - 1)
            const uint32_t w = (uint32_t)__shfl((int)mine, (int)k), op = w & 15u;
            const uint64_t len = w >> 4;
            if (pu_op_match(op) || op == 2) {
                const uint64_t j0 = lo > r ? lo - r : 0, j1 = hi > r ? (hi - r < len ? hi - r : len) : 0;
#pragma unroll 1
                for (uint64_t j = j0 + lane; j < j1; j += kWave) {
                    uint32_t plane = kPuDel;
                    if (op != 2) {
                        const uint32_t sb = pu_byte_by_dword(load, mis, s0 + (q + j) / 2), qb = pu_byte_by_dword(load, mis, q0 + q + j);
                        plane = pu_column_plane(pu_seq_code(sb, q + j), qb, min_baseq);
                    }
                    atomicAdd(&cnt[plane * kPuTile + (uint32_t)(r + j - t0)], 1u); // (lo <= r + j < hi: inside the tile)
                }
            } else if (op == 1 && lane == 0 && r > pos && r - 1 >= lo && r - 1 < hi) {
                atomicAdd(&cnt[kPuIns * kPuTile + (uint32_t)(r - 1 - t0)], 1u);
            }
            r += pu_op_ref(op) ? len : 0;
            q += pu_op_query(op) ? len : 0;
        }
    }
}

__global__ __launch_bounds__(256) void pu_tiles_kernel(const pileup_params P)
{
    __shared__ uint32_t cnt[kPuPlanes * kPuTile];
    __shared__ uint32_t s_visits;
    const uint32_t lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    const uint64_t t0 = P.O.begin + blockIdx.x * (uint64_t)kPuTile; // (the grid is ceil(np / kPuTile): t0 < O.end)
    const uint64_t t1 = t0 + kPuTile < P.O.end ? t0 + kPuTile : P.O.end;
    for (uint32_t k = threadIdx.x; k < kPuPlanes * kPuTile; k += 256)
        cnt[k] = 0;
    if (threadIdx.x == 0)
        s_visits = 0;
    __syncthreads();
    // the candidates: on a stream that is not in order the two bounds are any two places of [0, n], and end[] still names only
    // records that passed every test, so the walk stays inside record and tile
    const uint64_t i0 = uniform_u64(pu_first_above(P.pmax, P.n, t0)), i1 = uniform_u64(pu_first_at_or_behind(P.pos, P.n, t1));
    uint32_t visits = 0;
#pragma unroll 1
    for (uint64_t i = i0 + wave; i < i1; i += 4) {
        if (__builtin_amdgcn_readfirstlane(P.end[i]) <= t0)
            continue; // it does not take part, or ends in front of the tile
        const uint64_t off = uniform_u64(P.lines[i].offset);
        const uint32_t len = __builtin_amdgcn_readfirstlane(P.lines[i].len);
        pu_rec R;
        if (!pu_rec_read(P.stream, P.n_bytes, off, len, R))
            continue; // (counted by pu_records_kernel, which then wrote end[i] = 0)
        ++visits;
        pu_wave_walk(P, off, R, t0, t0, t1, cnt, lane);
    }
    if (lane == 0 && visits)
        atomicAdd(&s_visits, visits);
    __syncthreads();
    const uint32_t width = (uint32_t)(t1 - t0);
    const uint64_t at = t0 - P.O.begin;
#pragma unroll
    for (uint32_t p = 0; p < kPuPlanes; ++p)
        for (uint32_t x = threadIdx.x; x < width; x += 256)
            P.out[p * P.np + at + x] = cnt[p * kPuTile + x];
    if (threadIdx.x == 0 && s_visits)
        atomicAdd(&P.counts[kPuCntVisits], (unsigned long long)s_visits);
}

__global__ __launch_bounds__(256) void pu_summary_kernel(const pileup_params P)
{
    __shared__ unsigned long long part[4][4];
    unsigned long long covered = 0, sum = 0, top = 0, evidence = 0;
    for (uint64_t k = blockIdx.x * 256ull + threadIdx.x; k < P.np; k += gridDim.x * 256ull) {
        const uint32_t depth = pu_depth(P.out, P.np, k);
        covered += depth > 0;
        sum += depth;
        top = depth > top ? depth : top;
        evidence += (unsigned long long)depth + P.out[kPuIns * P.np + k] + P.out[kPuLowq * P.np + k];
    }
    covered = wave_sum(covered);
    sum = wave_sum(sum);
    top = wave_max(top);
    evidence = wave_sum(evidence);
    const uint32_t lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    if (lane == 0) {
        part[wave][0] = covered;
        part[wave][1] = sum;
        part[wave][2] = top;
        part[wave][3] = evidence;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t w = 1; w < 4; ++w) {
            covered += part[w][0];
            sum += part[w][1];
            top = part[w][2] > top ? part[w][2] : top;
            evidence += part[w][3];
        }
        if (covered)
            atomicAdd(&P.counts[kPuCntCovered], covered);
        if (sum)
            atomicAdd(&P.counts[kPuCntSumDepth], sum);
        if (top)
            atomicMax(&P.counts[kPuCntMaxDepth], top);
        if (evidence)
            atomicAdd(&P.counts[kPuCntEvidence], evidence);
    }
}

// ---- variant sites ----
struct pileup_sites_params
{
    const uint32_t *counts = nullptr; // the pileup: [8 * np]
    uint64_t np = 0, begin = 0;
    const uint8_t *ref = nullptr; // ranks; begin + np of them are read
    pu_site_opts O;
    uint32_t *flag = nullptr, *offs = nullptr; // [np]
    spm_pileup_site *dst = nullptr;
    uint64_t n_dst = 0;
    unsigned long long *n_sites = nullptr;
};

__global__ __launch_bounds__(256) void pu_sites_flag_kernel(const pileup_sites_params P)
{
    const uint64_t k = blockIdx.x * 256ull + threadIdx.x;
    bool site = false;
    if (k < P.np) {
        spm_pileup_site S;
        site = pu_site_of(P.counts, P.np, P.begin, k, P.ref[P.begin + k], P.O, S);
        P.flag[k] = site;
    }
    count_flagged(P.n_sites, site);
}

__global__ __launch_bounds__(256) void pu_sites_scatter_kernel(const pileup_sites_params P)
{
    const uint64_t k = blockIdx.x * 256ull + threadIdx.x;
    if (k >= P.np || !P.flag[k])
        return;
    spm_pileup_site S;
    if (pu_site_of(P.counts, P.np, P.begin, k, P.ref[P.begin + k], P.O, S) && P.offs[k] < P.n_dst)
        P.dst[P.offs[k]] = S;
}

using pileup_ptr = std::unique_ptr<spm_pileup, void (*)(spm_pileup *)>;
using pileup_sites_ptr = std::unique_ptr<spm_pileup_sites, void (*)(spm_pileup_sites *)>;

// what all three forms refuse before anything is read; O: the options the rule takes
static int pileup_check_args(const char *who, spm_ctx *ctx, const void *records, uint64_t n_bytes, const void *lines, uint64_t n_lines,
                             uint64_t ref_len, const spm_pileup_opts *opts, pu_opts &O)
{
    if (n_lines > 0xFFFFFFFFull) {
        SPM_SET_ERR(ctx, "%s: %llu records are more than 2^32 - 1 (not supported)", who, (unsigned long long)n_lines);
        return SPM_E_UNSUPPORTED;
    }
    if (ref_len > kPuMaxRefLen) {
        SPM_SET_ERR(ctx, "%s: ref_len %llu lies above 2^31, beyond what a BAM pos can name (not supported)", who, (unsigned long long)ref_len);
        return SPM_E_UNSUPPORTED;
    }
    O = pu_opts{};
    O.end = opts && opts->end ? opts->end : ref_len;
    O.begin = opts ? opts->begin : 0;
    const char *why = (!records && n_bytes)              ? "NULL records with n_record_bytes > 0"
                      : (!lines && n_lines)              ? "NULL lines with n_lines > 0"
                      : (n_lines == 0) != (n_bytes == 0) ? "records without lines, or lines without records"
                      : (opts && opts->flags)            ? "flags must be 0"
                      : (opts && (opts->reserved0 || opts->reserved1)) ? "reserved fields must be 0"
                      : (opts && opts->min_baseq > kPuMaxBaseq)        ? "min_baseq above 93"
                      : (O.begin > O.end || O.end > ref_len)           ? "the region is not begin <= end <= ref_len"
                                                                       : nullptr;
    if (why) {
        SPM_SET_ERR(ctx, "%s: %s", who, why);
        return SPM_E_INVALID;
    }
    O.exclude = (opts && opts->exclude_flags ? opts->exclude_flags : kPuDefaultExclude) | 0x4u;
    O.min_mapq = opts ? opts->min_mapq : 0;
    O.min_baseq = opts ? opts->min_baseq : 0;
    return SPM_OK;
}

static const char *const kPuDisagree = "records disagree with their line records or cannot be piled up (a line that leaves the stream, a "
                                       "block_size that is not len - 4, a name, CIGAR, seq or qual that leaves the record; a record that "
                                       "takes part with a refID other than 0, pos < 0, an end beyond ref_len, a CIGAR op above 8 or a CIGAR "
                                       "query length that is not l_seq; records out of coordinate order)";

// the stages of one call over a device stream that has passed pileup_check_args
static int pileup_run(const char *who, spm_ctx *ctx, const uint8_t *d_stream, uint64_t n_bytes, const spm_sam_line *d_lines, uint32_t n,
                      uint64_t ref_len, const pu_opts &O, spm_pileup **out)
{
    const clk::time_point t_call = clk::now();
    SPM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    dev_scratch keep;
    hip_events<5> ev; // before records, behind records, scan, tiles, summary
    SPM_HIP_CHECK(ctx, ev.create());
    pileup_params P;
    P.stream = d_stream;
    P.n_bytes = n_bytes;
    P.lines = d_lines;
    P.n = n;
    P.ref_len = ref_len;
    P.O = O;
    P.np = O.end - O.begin;
    pileup_ptr R(new spm_pileup, spm_hip_pileup_destroy);
    R->ctx = ctx;
    R->begin = O.begin;
    R->n = P.np;
    SPM_HIP_CHECK(ctx, keep.alloc(&P.counts, kPuCnts * 8));
    SPM_HIP_CHECK(ctx, hipMemsetAsync(P.counts, 0, kPuCnts * 8, st));
    void *d_tmp = nullptr;
    size_t tmp_bytes = 0;
    if (n) {
        SPM_HIP_CHECK(ctx, scan_u32_tmp_bytes(ctx, n, &tmp_bytes));
        SPM_HIP_CHECK(ctx, keep.alloc(&d_tmp, std::max<size_t>(tmp_bytes, 1)));
        SPM_HIP_CHECK(ctx, keep.alloc(&P.pos, (size_t)n * 4));
        SPM_HIP_CHECK(ctx, keep.alloc(&P.end, (size_t)n * 4));
        SPM_HIP_CHECK(ctx, keep.alloc(&P.pmax, (size_t)n * 4));
    }
    if (P.np) {
        SPM_HIP_CHECK(ctx, hipMalloc(&R->d, kPuPlanes * P.np * sizeof(uint32_t)));
        P.out = R->d;
    }
    SPM_HIP_CHECK(ctx, hipEventRecord(ev[0], st));
    if (n)
        SPM_HIP_CHECK(ctx, launch_1d(ctx, pu_records_kernel, n, P));
    SPM_HIP_CHECK(ctx, hipEventRecord(ev[1], st));
    if (n)
        SPM_HIP_CHECK(ctx, inclusive_max_u32(ctx, d_tmp, tmp_bytes, P.end, P.pmax, n));
    SPM_HIP_CHECK(ctx, hipEventRecord(ev[2], st));
    if (P.np) { // (without records the tiles find no candidates and store zeros)
        hipLaunchKernelGGL(pu_tiles_kernel, dim3((unsigned)((P.np + kPuTile - 1) / kPuTile)), dim3(256), 0, st, P);
        SPM_HIP_CHECK(ctx, hipGetLastError());
    }
    SPM_HIP_CHECK(ctx, hipEventRecord(ev[3], st));
    if (P.np) {
        const uint64_t blocks = std::min<uint64_t>((P.np + 255) / 256, 2048);
        hipLaunchKernelGGL(pu_summary_kernel, dim3((unsigned)blocks), dim3(256), 0, st, P);
        SPM_HIP_CHECK(ctx, hipGetLastError());
    }
    SPM_HIP_CHECK(ctx, hipEventRecord(ev[4], st));
    SPM_HIP_CHECK(ctx, read_counts(ctx, P.counts, kPuCnts));
    const unsigned long long *c = ctx->h_counters;
    if (c[kPuCntBad]) {
        SPM_SET_ERR(ctx, "%s: %llu %s; ref_len %llu; nothing was returned", who, c[kPuCntBad], kPuDisagree, (unsigned long long)ref_len);
        return SPM_E_INVALID;
    }
    spm_pileup_stats &S = R->stats;
    hipEventElapsedTime(&S.ms_records, ev[0], ev[1]);
    hipEventElapsedTime(&S.ms_scan, ev[1], ev[2]);
    hipEventElapsedTime(&S.ms_tiles, ev[2], ev[3]);
    hipEventElapsedTime(&S.ms_summary, ev[3], ev[4]);
    S.ms_total = S.ms_records + S.ms_scan + S.ms_tiles + S.ms_summary;
    S.tile_positions = kPuTile;
    S.n_records = n;
    S.n_taking_part = c[kPuCntTaking];
    S.n_evidence = c[kPuCntEvidence];
    S.n_covered = c[kPuCntCovered];
    S.sum_depth = c[kPuCntSumDepth];
    S.max_depth = c[kPuCntMaxDepth];
    S.n_tile_visits = c[kPuCntVisits];
    S.ms_host = ms_since(t_call);
    if (spm_trace_on())
        fprintf(stderr, "[spm_hip] bam pileup: %u records (%llu take part, %llu tile visits), %llu positions (%llu covered, depth up to "
                        "%llu): device %.3f ms (records %.3f, scan %.3f, tiles %.3f, summary %.3f), %.3f ms in all\n", n, c[kPuCntTaking],
                c[kPuCntVisits], (unsigned long long)P.np, c[kPuCntCovered], c[kPuCntMaxDepth], S.ms_total, S.ms_records, S.ms_scan, S.ms_tiles,
                S.ms_summary, S.ms_host);
    *out = R.release();
    return SPM_OK;
}

static bool pileup_site_opts(const spm_pileup_site_opts *opts, pu_site_opts &O)
{
    O = pu_site_opts{};
    if (!opts)
        return true;
    O.min_depth = opts->min_depth;
    O.min_alt = opts->min_alt;
    O.min_alt_permille = opts->min_alt_permille;
    return opts->flags == 0;
}

} // namespace spm_hip

extern "C" int spm_hip_bam_pileup(spm_bam *b, const spm_pileup_opts *opts, spm_pileup **out)
{
    static const char *const who = "spm_hip_bam_pileup";
    if (out)
        *out = nullptr;
    if (!b || !out)
        return SPM_E_INVALID;
    spm_ctx *ctx = b->ctx;
    pu_opts O;
    SPM_TRY(pileup_check_args(who, ctx, b->d_records, b->n_record_bytes, b->d_lines, b->n_lines, b->ref_len, opts, O));
    return pileup_run(who, ctx, b->d_records, b->n_record_bytes, b->d_lines, (uint32_t)b->n_lines, b->ref_len, O, out);
}

extern "C" int spm_hip_bam_pileup_records(spm_ctx *ctx, const void *device_records, uint64_t n_record_bytes, const void *device_lines,
                                          uint64_t n_lines, uint64_t ref_len, const spm_pileup_opts *opts, spm_pileup **out)
{
    static const char *const who = "spm_hip_bam_pileup_records";
    if (out)
        *out = nullptr;
    if (!ctx || !out) {
        SPM_SET_ERR(ctx, "%s: NULL %s", who, !ctx ? "ctx" : "out");
        return SPM_E_INVALID;
    }
    pu_opts O;
    SPM_TRY(pileup_check_args(who, ctx, device_records, n_record_bytes, device_lines, n_lines, ref_len, opts, O));
    return pileup_run(who, ctx, static_cast<const uint8_t *>(device_records), n_record_bytes, static_cast<const spm_sam_line *>(device_lines),
                      (uint32_t)n_lines, ref_len, O, out);
}

extern "C" int spm_hip_bam_pileup_host(const void *records, uint64_t n_record_bytes, const spm_sam_line *lines, uint64_t n_lines,
                                       uint64_t ref_len, const spm_pileup_opts *opts, uint32_t *counts)
{
    static const char *const who = "spm_hip_bam_pileup_host";
    pu_opts O;
    SPM_TRY(pileup_check_args(who, nullptr, records, n_record_bytes, lines, n_lines, ref_len, opts, O));
    if (!counts && O.end > O.begin) {
        SPM_SET_ERR((spm_ctx *)nullptr, "%s: NULL counts with a region that is not empty", who);
        return SPM_E_INVALID;
    }
    if (!pileup_serial(static_cast<const uint8_t *>(records), n_record_bytes, lines, n_lines, ref_len, O, counts)) {
        SPM_SET_ERR((spm_ctx *)nullptr, "%s: %s", who, kPuDisagree);
        return SPM_E_INVALID;
    }
    return SPM_OK;
}

extern "C" int spm_hip_pileup_view(spm_pileup *p, const uint32_t **counts, uint64_t *n_positions)
{
    if (!p)
        return SPM_E_INVALID;
    SPM_TRY(handle_download(p->ctx, p->have_host, view_part{p->d, kPuPlanes * p->n, p->host}));
    out_if(counts, (const uint32_t *)p->host.data());
    out_if(n_positions, p->n);
    return SPM_OK;
}

extern "C" int spm_hip_pileup_device(spm_pileup *p, const void **counts, uint64_t *n_positions)
{
    if (!p)
        return SPM_E_INVALID;
    out_if(counts, (const void *)p->d);
    out_if(n_positions, p->n);
    return SPM_OK;
}

extern "C" int spm_hip_pileup_stats(const spm_pileup *p, spm_pileup_stats *out) { return stats_out(p ? &p->stats : nullptr, out); }

extern "C" void spm_hip_pileup_destroy(spm_pileup *p)
{
    if (p)
        handle_destroy(p, {p->d});
}

extern "C" int spm_hip_pileup_sites(spm_pileup *p, const spm_text *reference, const spm_pileup_site_opts *opts, spm_pileup_sites **out)
{
    static const char *const who = "spm_hip_pileup_sites";
    if (out)
        *out = nullptr;
    if (!p || !out)
        return SPM_E_INVALID;
    spm_ctx *ctx = p->ctx;
    pileup_sites_params P;
    const char *why = !reference                            ? "NULL reference"
                      : reference->ctx != ctx               ? "the reference belongs to another context"
                      : reference->sigma != 4               ? "the reference is not dna4"
                      : reference->n < p->begin + p->n      ? "the reference is shorter than the pileup's end"
                      : !pileup_site_opts(opts, P.O)        ? "flags must be 0"
                                                            : nullptr;
    if (why) {
        SPM_SET_ERR(ctx, "%s: %s", who, why);
        return SPM_E_INVALID;
    }
    SPM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    pileup_sites_ptr R(new spm_pileup_sites, spm_hip_pileup_sites_destroy);
    R->ctx = ctx;
    if (p->n) {
        hipStream_t st = ctx->stream;
        dev_scratch keep;
        void *d_tmp = nullptr;
        size_t tmp_bytes = 0;
        P.counts = p->d;
        P.np = p->n;
        P.begin = p->begin;
        P.ref = reference->d;
        SPM_HIP_CHECK(ctx, scan_u32_tmp_bytes(ctx, P.np, &tmp_bytes));
        SPM_HIP_CHECK(ctx, keep.alloc(&d_tmp, std::max<size_t>(tmp_bytes, 1)));
        SPM_HIP_CHECK(ctx, keep.alloc(&P.flag, (size_t)P.np * 4));
        SPM_HIP_CHECK(ctx, keep.alloc(&P.offs, (size_t)P.np * 4));
        SPM_HIP_CHECK(ctx, keep.alloc(&P.n_sites, 8));
        SPM_HIP_CHECK(ctx, hipMemsetAsync(P.n_sites, 0, 8, st));
        SPM_HIP_CHECK(ctx, launch_1d(ctx, pu_sites_flag_kernel, P.np, P));
        SPM_HIP_CHECK(ctx, exclusive_sum_u32(ctx, d_tmp, tmp_bytes, P.flag, P.offs, P.np));
        SPM_HIP_CHECK(ctx, read_counts(ctx, P.n_sites, 1)); // the one read-back: the size of the result
        R->n = P.n_dst = ctx->h_counters[0];
        if (R->n) {
            SPM_HIP_CHECK(ctx, hipMalloc(&R->d, R->n * sizeof(spm_pileup_site)));
            P.dst = R->d;
            SPM_HIP_CHECK(ctx, launch_1d(ctx, pu_sites_scatter_kernel, P.np, P));
            SPM_HIP_CHECK(ctx, hipStreamSynchronize(st)); // (the scratch goes with this scope)
        }
    }
    *out = R.release();
    return SPM_OK;
}

extern "C" int spm_hip_pileup_sites_view(spm_pileup_sites *s, const spm_pileup_site **sites, uint64_t *n)
{
    if (!s)
        return SPM_E_INVALID;
    SPM_TRY(handle_download(s->ctx, s->have_host, view_part{s->d, s->n, s->host}));
    out_if(sites, (const spm_pileup_site *)s->host.data());
    out_if(n, s->n);
    return SPM_OK;
}

extern "C" int spm_hip_pileup_sites_device(spm_pileup_sites *s, const void **sites, uint64_t *n)
{
    if (!s)
        return SPM_E_INVALID;
    out_if(sites, (const void *)s->d);
    out_if(n, s->n);
    return SPM_OK;
}

extern "C" void spm_hip_pileup_sites_destroy(spm_pileup_sites *s)
{
    if (s)
        handle_destroy(s, {s->d});
}

extern "C" int spm_hip_pileup_sites_host(const uint32_t *counts, uint64_t begin, uint64_t n_positions, const uint8_t *ref_ranks,
                                         uint64_t ref_len, const spm_pileup_site_opts *opts, spm_pileup_site *dst, uint64_t cap, uint64_t *n)
{
    static const char *const who = "spm_hip_pileup_sites_host";
    pu_site_opts O;
    const char *why = !n                                          ? "NULL n"
                      : (!counts || !ref_ranks) && n_positions    ? "NULL counts or ref_ranks with n_positions > 0"
                      : begin > ref_len || n_positions > ref_len - begin ? "the reference is shorter than the pileup's end"
                      : !dst && cap                               ? "NULL dst with cap > 0"
                      : !pileup_site_opts(opts, O)                ? "flags must be 0"
                                                                  : nullptr;
    if (why) {
        SPM_SET_ERR((spm_ctx *)nullptr, "%s: %s", who, why);
        return SPM_E_INVALID;
    }
    std::vector<spm_pileup_site> sites;
    pileup_sites_serial(counts, begin, n_positions, ref_ranks, O, sites);
    *n = sites.size();
    if (sites.size() > cap) {
        SPM_SET_ERR((spm_ctx *)nullptr, "%s: %llu sites need more than cap %llu", who, (unsigned long long)sites.size(), (unsigned long long)cap);
        return SPM_E_OVERFLOW;
    }
    std::copy(sites.begin(), sites.end(), dst);
    return SPM_OK;
}

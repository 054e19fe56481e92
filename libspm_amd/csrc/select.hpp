// select.hpp -- the kernels of hit selection (spm_hip_hits_select / spm_hip_records_select; contract in spm_hip.h, scheme in
// DESIGN.md 4.7).  gfx950.  The records are ordered by a radix sort of (key, index) pairs, key = pattern << pos_bits |
// (pos - bias); then
//   select_loci_kernel     one lane per sorted record: is a record of the same pattern (and segment) within the window
//                          better?  Neighbours inside the window are contiguous in sorted order, so a tile of keys and
//                          scores with a halo on either side is staged in LDS; also the per-pattern score minima;
//   select_compact_kernel  the stratum test, and the stable compaction of the kept records into the new hit block through an
//                          exclusive scan of the keep flags (the order IS the contract: no slot atomics).
// With SPM_SELECT_STRANDS the minimum is per read = pattern >> shift: the strand is the pattern's lowest bit, so
// a read's two strands are adjacent runs of the sorted order.  shift = 0 is the selection per pattern, expression for expression.
// Also here: select_params, the keys and range kernels, sel_final.  Staging, walks, flag functor: select_walk.hpp; the kept count
// and the segmented min-scan: wave.hpp.
#pragma once

#include <hip/hip_runtime.h>

#include "common.hpp"
#include "select_plan.hpp"
#include "select_walk.hpp"

namespace spm_hip
{

struct select_params
{
    const spm_hit *recs = nullptr;            // the source's records, in their arrival order
    unsigned long long *keys = nullptr;       // [n] sorted keys
    uint32_t *idx = nullptr;                  // [n] record index of sorted entry i
    uint32_t n = 0;
    uint32_t pos_bits = 0;                    // key >> pos_bits = pattern (pos_bits == 64: one pattern, index 0)
    unsigned long long pos_mask = 0;          // key & pos_mask = pos - bias
    unsigned long long bias = 0;
    uint32_t loci = 0;
    uint32_t best = 0;
    uint32_t shift = 0;                       // BEST's minimum is taken per pattern >> shift (1: SPM_SELECT_STRANDS, per read)
    uint32_t window = 0;                      // SPM_SELECT_WINDOW_K: k_tab[pattern]
    const int32_t *k_tab = nullptr;
    uint32_t halo = 0;                        // <= kSelHaloCap
    const unsigned long long *segs = nullptr; // segmented sources: n_segs + 1 ascending offsets, text coordinates
    unsigned long long n_segs = 0;
    unsigned long long seg_bias = 0;          // (pos - bias) + seg_bias = pos - pos_offset
    uint32_t seg_myers = 0;                   // a record at p belongs to the segment of symbol p - 1 (Myers: pos is an end)
    long long strata = 0;
    // out
    uint8_t *keep = nullptr;                  // [n] LOCI's verdict
    int32_t *score = nullptr;                 // [n] scores in sorted order
    int32_t *minima = nullptr;                // [min_slots] minimal score per pattern >> shift (BEST only; preset to INT_MAX)
    unsigned long long *counts = nullptr;     // [0] records LOCI kept, [1] records of the result
};

__device__ __forceinline__ uint32_t sel_pattern(const select_params &P, unsigned long long key)
{
    return P.pos_bits < 64 ? (uint32_t)(key >> P.pos_bits) : 0u;
}

// one lane per record: key and index, ready for the sort
__global__ __launch_bounds__(256) void select_keys_kernel(const spm_hit *__restrict__ recs, unsigned long long *__restrict__ keys,
                                                            uint32_t *__restrict__ idx, uint32_t n, uint32_t pos_bits,
                                                            unsigned long long bias)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n)
        return;
    const uint4 r = reinterpret_cast<const uint4 *>(recs)[i];
    const unsigned long long pos = ((unsigned long long)r.y << 32 | r.x) - bias;
    keys[i] = (pos_bits < 64 ? (unsigned long long)r.z << pos_bits : 0ull) | pos;
    idx[i] = i;
}

// spm_hip_records_select: the range of what a raw buffer holds -- out[0] = min pos, out[1] = max pos (both as signed
// values, sign bit flipped so that unsigned atomics order them), out[2] = max pattern
__global__ __launch_bounds__(256) void select_range_kernel(const spm_hit *__restrict__ recs, uint32_t n,
                                                             unsigned long long *__restrict__ out)
{
    constexpr unsigned long long kSign = 1ull << 63;
    unsigned long long lo = ~0ull, hi = 0, pat = 0;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const uint4 r = reinterpret_cast<const uint4 *>(recs)[i];
        const unsigned long long pos = ((unsigned long long)r.y << 32 | r.x) ^ kSign;
        lo = pos < lo ? pos : lo;
        hi = pos > hi ? pos : hi;
        pat = r.z > pat ? r.z : pat;
    }
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned long long l2 = __shfl_xor(lo, d), h2 = __shfl_xor(hi, d), p2 = __shfl_xor(pat, d);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
        pat = p2 > pat ? p2 : pat;
    }
    if ((threadIdx.x & 63) == 0) {
        atomicMin(&out[0], lo);
        atomicMax(&out[1], hi);
        atomicMax(&out[2], pat);
    }
}

// One lane per sorted record.  LDS holds the keys and scores of the tile and of `halo` records on either side; a lane whose
// window reaches further reads global memory (needles with k > 32).  Here: the pattern as the group, the segment range.
__global__ __launch_bounds__(kSelTile) void select_loci_kernel(const select_params P)
{
    __shared__ unsigned long long s_key[kSelLdsEntries];
    __shared__ int32_t s_score[kSelLdsEntries];
    const auto score_of = [&](long long j) { return P.recs[P.idx[j]].score; };
    const sel_tile T = sel_stage_tile(s_key, s_score, P.keys, P.n, P.halo, score_of);

    const long long i = (long long)blockIdx.x * kSelTile + threadIdx.x;
    const bool valid = i < T.n;
    uint32_t pat = 0xFFFFFFFFu;
    int32_t sc = 0x7FFFFFFF;
    bool kept = false;
    if (valid) {
        const unsigned long long key = s_key[P.halo + threadIdx.x];
        sc = s_score[P.halo + threadIdx.x];
        pat = sel_pattern(P, key);
        P.score[i] = sc;
        kept = true;
        const unsigned long long w = !P.loci ? 0ull : P.window == SPM_SELECT_WINDOW_K ? (unsigned long long)max(P.k_tab[pat], 0) : P.window;
        if (w) {
            const unsigned long long rel = key & P.pos_mask;
            // the record's segment, as the closed range of positions (pos - pos_offset) its records can have
            unsigned long long p_lo = 0, p_hi = ~0ull;
            if (P.segs) {
                const unsigned long long p = rel + P.seg_bias;
                const unsigned long long sym = P.seg_myers && p ? p - 1 : p; // the symbol that decides the segment
                unsigned long long a = 0, b = P.n_segs;                       // last s with segs[s] <= sym (0 if none)
                while (b - a > 1) {
                    const unsigned long long mid = a + (b - a) / 2;
                    if (P.segs[mid] <= sym)
                        a = mid;
                    else
                        b = mid;
                }
                // (positions outside the table count to the first / last segment)
                p_lo = a == 0 ? 0ull : P.segs[a] + P.seg_myers;
                p_hi = a + 1 == P.n_segs ? ~0ull : P.segs[a + 1] - 1 + P.seg_myers;
            }
            kept = sel_walk_keeps(
                s_key, s_score, P.keys, T, i, pat, rel, sc, P.pos_mask, w, [&](unsigned long long k) { return sel_pattern(P, k); },
                score_of, [&](unsigned long long rj) { return rj + P.seg_bias >= p_lo && rj + P.seg_bias <= p_hi; });
        }
        P.keep[i] = kept ? 1 : 0;
    }
    count_flagged(&P.counts[0], kept);
    // per-pattern minima: the last lane of every run issues the one atomicMin of that wave and pattern (with a shift: of
    // that read, whose two strands are adjacent runs of the sorted order)
    if (P.best) {
        const uint32_t grp = pat >> P.shift;
        run_min<int32_t> m{sc};
        const bool run_ends = wave_run_scan(grp, m);
        if (valid && (run_ends || i + 1 >= T.n))
            atomicMin(&P.minima[grp], m.v);
    }
}

// the final flag of sorted record i: the minimum it is measured against is its pattern's (its read's)
__device__ __forceinline__ uint32_t sel_final(const select_params &P, uint32_t i)
{
    return sel_final_flag(P, i, [&](uint32_t r) { return sel_pattern(P, P.keys[r]) >> P.shift; });
}

// offs: exclusive scan of the final flags.  A kept record travels as one 16-byte load and one 16-byte store.
__global__ __launch_bounds__(256) void select_compact_kernel(const select_params P, const uint32_t *__restrict__ offs,
                                                               spm_hit *__restrict__ out,
                                                               unsigned long long *__restrict__ hit_counter)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= P.n)
        return;
    const uint32_t f = sel_final(P, i);
    const uint32_t o = offs[i];
    if (f)
        reinterpret_cast<uint4 *>(out)[o] = reinterpret_cast<const uint4 *>(P.recs)[P.idx[i]];
    if (i == P.n - 1) {
        P.counts[1] = (unsigned long long)o + f;
        *hit_counter = (unsigned long long)o + f;
    }
}

} // namespace spm_hip

// jst_select.hpp -- the kernels of pan-genome hit selection (spm_hip_jst_hits_select / spm_hip_jst_records_select; contract
// in spm_hip.h, scheme in DESIGN.md 4.7).  gfx950.  The siblings of select.hpp for the 24-byte spm_jst_hit: the records are
// ordered by a radix sort of (key, index) pairs, key = haplotype << (pat_bits + pos_bits) | pattern << pos_bits | pos, so
// that key >> pos_bits names the group (haplotype, pattern) whose records see each other; then
//   jst_select_loci_kernel     one lane per sorted record: is a record of the same group within the window better?  Also the
//                              head flag of every group;
//   jst_select_minima_kernel   BEST: the minimal score of every group, into an array indexed by the group's number (the
//                              exclusive sum of the head flags) -- or, with ACROSS, by the pattern;
//   jst_select_compact_kernel  the stratum test and the stable compaction of the kept records, three 8-byte words each.
// With SPM_SELECT_STRANDS the minimum's group is group >> shift, (haplotype, read) -- or with ACROSS the read -- since the
// strand is the group's lowest bit; LOCI's group stays (haplotype, pattern).
// Also here: jst_select_params, the keys and range kernels, the group numbering (jsel_gid, jsel_min_slot), sel_final.
// Staging, walks and the flag functor are select_walk.hpp's, shared with select.hpp; the kept count and the segmented
// min-scan are wave.hpp's.
#pragma once

#include <hip/hip_runtime.h>

#include "common.hpp"
#include "select_plan.hpp"
#include "select_walk.hpp"

namespace spm_hip
{

struct jst_select_params
{
    const unsigned long long *recs = nullptr; // the source's records as 8-byte words, three each, in their arrival order:
                                              // pos | pattern << 32 + haplotype | reserved << 32 + score
    unsigned long long *keys = nullptr;       // [n] sorted keys
    uint32_t *idx = nullptr;                  // [n] record index of sorted entry i
    const int32_t *score_in = nullptr;        // [n] scores in arrival order (the keys kernel wrote them)
    uint32_t n = 0;
    uint32_t pos_bits = 0;                    // key >> pos_bits = group (pos_bits == 64: one group, number 0)
    unsigned long long pos_mask = 0;
    uint32_t pat_mask = 0;                    // group & pat_mask = pattern
    uint32_t loci = 0, best = 0, across = 0;
    uint32_t shift = 0;                       // BEST's minimum is taken per group >> shift (1: SPM_SELECT_STRANDS, per read)
    uint32_t window = 0;                      // SPM_SELECT_WINDOW_K: k_tab[pattern]
    const int32_t *k_tab = nullptr;
    uint32_t halo = 0;                        // <= kSelHaloCap
    long long strata = 0;
    // out
    uint8_t *keep = nullptr;                  // [n] LOCI's verdict
    uint8_t *head = nullptr;                  // [n] 1 where a group >> shift begins
    int32_t *score = nullptr;                 // [n] scores in sorted order
    const uint32_t *gid = nullptr;            // [n] exclusive sum of head (BEST without ACROSS)
    int32_t *minima = nullptr;                // BEST: minimal score per group number / per pattern (preset to INT_MAX)
    unsigned long long *counts = nullptr;     // [0] records LOCI kept, [1] records of the result
};

__device__ __forceinline__ unsigned long long jsel_group(const jst_select_params &P, unsigned long long key)
{
    return P.pos_bits < 64 ? key >> P.pos_bits : 0ull;
}

__device__ __forceinline__ unsigned long long jsel_key(unsigned long long w_pos, unsigned long long w_hp, uint32_t pos_bits,
                                                       uint32_t pat_bits)
{
    const unsigned long long hap = w_hp & 0xFFFFFFFFull, pat = w_hp >> 32;
    const unsigned long long grp = pat_bits < 64 ? hap << pat_bits | pat : pat; // (pat_bits <= 32 in fact)
    return (pos_bits < 64 ? grp << pos_bits : 0ull) | w_pos;
}

// One lane per record.  The 256 records of a workgroup are 768 contiguous 8-byte words (a wave's share: 1 536 bytes): they
// are read as such, three coalesced loads per lane, and handed to their lanes through LDS.  Key, index and score leave in
// arrival order: the later stages gather a 4-byte score through the sorted index, never a record.
__global__ __launch_bounds__(256) void jst_select_keys_kernel(const unsigned long long *__restrict__ recs,
                                                                unsigned long long *__restrict__ keys, uint32_t *__restrict__ idx,
                                                                int32_t *__restrict__ score, uint32_t n, uint32_t pos_bits,
                                                                uint32_t pat_bits)
{
    __shared__ unsigned long long s_w[3 * 256];
    const unsigned long long base = (unsigned long long)blockIdx.x * 256ull;
    const unsigned long long n_words = 3ull * n;
#pragma unroll
    for (uint32_t r = 0; r < 3; ++r) {
        const unsigned long long w = base * 3ull + r * 256u + threadIdx.x;
        if (w < n_words)
            s_w[r * 256u + threadIdx.x] = recs[w];
    }
    __syncthreads();
    const unsigned long long i = base + threadIdx.x;
    if (i >= n)
        return;
    const unsigned long long w_pos = s_w[3 * threadIdx.x], w_hp = s_w[3 * threadIdx.x + 1], w_sc = s_w[3 * threadIdx.x + 2];
    keys[i] = jsel_key(w_pos, w_hp, pos_bits, pat_bits);
    idx[i] = (uint32_t)i;
    score[i] = (int32_t)(uint32_t)w_sc;
}

// spm_hip_jst_records_select: the range of what a raw buffer holds -- out[0] = max haplotype, out[1] = max pattern,
// out[2] = max pos.  Grid-stride; one atomic triple per wave.
__global__ __launch_bounds__(256) void jst_select_range_kernel(const unsigned long long *__restrict__ recs, uint32_t n,
                                                                 unsigned long long *__restrict__ out)
{
    unsigned long long hap = 0, pat = 0, pos = 0;
    for (unsigned long long i = blockIdx.x * 256ull + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256ull) {
        const unsigned long long w_pos = recs[3 * i], w_hp = recs[3 * i + 1];
        const unsigned long long h = w_hp & 0xFFFFFFFFull, p = w_hp >> 32;
        pos = w_pos > pos ? w_pos : pos;
        hap = h > hap ? h : hap;
        pat = p > pat ? p : pat;
    }
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned long long h2 = __shfl_xor(hap, d), p2 = __shfl_xor(pat, d), q2 = __shfl_xor(pos, d);
        hap = h2 > hap ? h2 : hap;
        pat = p2 > pat ? p2 : pat;
        pos = q2 > pos ? q2 : pos;
    }
    if ((threadIdx.x & 63) == 0) {
        atomicMax(&out[0], hap);
        atomicMax(&out[1], pat);
        atomicMax(&out[2], pos);
    }
}

// One lane per sorted record, as select_loci_kernel and from the same pieces (select_walk.hpp).  The group test is
// key >> pos_bits, haplotype AND pattern: records of neighbouring haplotypes never see each other, and every position is
// allowed (no segment notion).
__global__ __launch_bounds__(kSelTile) void jst_select_loci_kernel(const jst_select_params P)
{
    __shared__ unsigned long long s_key[kSelLdsEntries];
    __shared__ int32_t s_score[kSelLdsEntries];
    const auto score_of = [&](long long j) { return P.score_in[P.idx[j]]; };
    const sel_tile T = sel_stage_tile(s_key, s_score, P.keys, P.n, P.halo, score_of);

    const long long i = (long long)blockIdx.x * kSelTile + threadIdx.x;
    bool kept = false;
    if (i < T.n) {
        const unsigned long long key = s_key[P.halo + threadIdx.x];
        const int32_t sc = s_score[P.halo + threadIdx.x];
        const unsigned long long grp = jsel_group(P, key);
        P.score[i] = sc;
        kept = true;
        if (i == 0)
            P.head[i] = 1;
        else {
            const unsigned long long kp = i - 1 >= T.lds0 ? s_key[i - 1 - T.lds0] : P.keys[i - 1];
            P.head[i] = (jsel_group(P, kp) >> P.shift) != (grp >> P.shift) ? 1 : 0;
        }
        const unsigned long long w = !P.loci                            ? 0ull
                                     : P.window == SPM_SELECT_WINDOW_K ? (unsigned long long)max(P.k_tab[(uint32_t)grp & P.pat_mask], 0)
                                                                       : P.window;
        if (w)
            kept = sel_walk_keeps(
                s_key, s_score, P.keys, T, i, grp, key & P.pos_mask, sc, P.pos_mask, w,
                [&](unsigned long long k) { return jsel_group(P, k); }, score_of, [](unsigned long long) { return true; });
        P.keep[i] = kept ? 1 : 0;
    }
    count_flagged(&P.counts[0], kept);
}

// the number of record i's group among the groups of the sorted list
__device__ __forceinline__ uint32_t jsel_gid(const jst_select_params &P, uint32_t i) { return P.gid[i] + P.head[i] - 1u; }
// where the minimum that record i is measured against lives
__device__ __forceinline__ uint32_t jsel_min_slot(const jst_select_params &P, uint32_t i)
{
    return P.across ? ((uint32_t)jsel_group(P, P.keys[i]) & P.pat_mask) >> P.shift : jsel_gid(P, i);
}

// BEST: the last lane of every run of one group in a wave (wave_run_scan) issues the one atomicMin of that wave and group.  A
// table of n_haplotypes x n_patterns minima would not fit; the groups that occur are numbered instead, and there are at
// most n of them.
__global__ __launch_bounds__(256) void jst_select_minima_kernel(const jst_select_params P)
{
    const unsigned long long i = blockIdx.x * 256ull + threadIdx.x;
    const bool valid = i < P.n;
    unsigned long long grp = ~0ull;
    int32_t sc = 0x7FFFFFFF;
    if (valid) {
        grp = jsel_group(P, P.keys[i]) >> P.shift;
        sc = P.score[i];
    }
    run_min<int32_t> m{sc};
    const bool run_ends = wave_run_scan(grp, m);
    if (valid && (run_ends || i + 1 >= P.n))
        atomicMin(&P.minima[jsel_min_slot(P, (uint32_t)i)], m.v);
}

// the final flag of sorted record i
__device__ __forceinline__ uint32_t sel_final(const jst_select_params &P, uint32_t i)
{
    return sel_final_flag(P, i, [&](uint32_t r) { return jsel_min_slot(P, r); });
}
struct jsel_head_op
{
    const uint8_t *head;
    __device__ __forceinline__ uint32_t operator()(uint32_t i) const { return head[i]; }
};

// offs: exclusive scan of the final flags.  A kept record travels as three 8-byte words.  The last lane writes the counts
// the host reads back.
__global__ __launch_bounds__(256) void jst_select_compact_kernel(const jst_select_params P, const uint32_t *__restrict__ offs,
                                                                   unsigned long long *__restrict__ out)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= P.n)
        return;
    const uint32_t f = sel_final(P, i);
    const uint32_t o = offs[i];
    if (f) {
        const unsigned long long *src = P.recs + 3ull * P.idx[i];
        unsigned long long *dst = out + 3ull * o;
        const unsigned long long a = src[0], b = src[1], c = src[2];
        dst[0] = a;
        dst[1] = b;
        dst[2] = c;
    }
    if (i == P.n - 1)
        P.counts[1] = (unsigned long long)o + f;
}

} // namespace spm_hip

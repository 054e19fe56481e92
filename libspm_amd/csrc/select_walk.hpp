// select_walk.hpp -- the device pieces that the two selections share (select.hpp: 16-byte spm_hit; jst_select.hpp: 24-byte
// spm_jst_hit).  gfx950.  Holds the tile staging and the two window walks of LOCI, and the final flag with its
// functor; the kept count and the segmented min-scan of BEST are wave.hpp's (count_flagged, wave_run_scan over a run_min).
// __device__ __forceinline__ templates over functors, no class hierarchy: every kernel stays in its own header and passes
// what differs --
//   group_of(key)  the group whose records see each other: the pattern, or (haplotype, pattern)
//   score_of(j)    the score of sorted entry j, from global memory (staging, and a walk that leaves the halo)
//   allowed(rel)   may a neighbour at this position suppress?  (the plain selection's segment range; pan-genome: always)
//   slot_of(i)     where the minimum that record i is measured against lives
#pragma once

#include <hip/hip_runtime.h>

#include "select_plan.hpp"
#include "wave.hpp"

namespace spm_hip
{

constexpr uint32_t kSelLdsEntries = kSelTile + 2 * kSelHaloCap; // keys and scores a loci kernel holds in LDS

struct sel_tile // where a workgroup's staged records sit in the sorted list
{
    long long n;       // records in the list
    long long lds0;    // sorted index of s_key[0] (negative in the first tile)
    long long lds_end; // one past the last staged index
};

// Stages the keys and scores of the workgroup's tile and of `halo` (<= kSelHaloCap) records on either side, and
// synchronises.  Entry t of the LDS arrays is sorted index lds0 + t; the lane's own record is entry halo + threadIdx.x.
template <class ScoreOf>
__device__ __forceinline__ sel_tile sel_stage_tile(unsigned long long *s_key, int32_t *s_score,
                                                   const unsigned long long *__restrict__ keys, uint32_t n, uint32_t halo,
                                                   ScoreOf score_of)
{
    sel_tile T;
    T.n = n;
    T.lds0 = (long long)blockIdx.x * kSelTile - halo;
    T.lds_end = T.lds0 + kSelTile + 2 * halo;
    for (uint32_t t = threadIdx.x; t < kSelTile + 2 * halo; t += kSelTile) {
        const long long j = T.lds0 + t;
        if (j >= 0 && j < T.n) {
            s_key[t] = keys[j];
            s_score[t] = score_of(j);
        }
    }
    __syncthreads();
    return T;
}

// LOCI's verdict on sorted record i = (group grp, position rel = key & pos_mask, score sc) with window w > 0: false iff a
// record of the same group within w, at an allowed position, is better -- the contract's literal rule (spm_hip.h):
// (score', pos') < (score, pos).  Positions to the right are not smaller, so there only a strictly smaller score is better.
// Two records of one group at ONE position with equal scores both stay: the plain selection has always treated them so, and
// pan-genome input never holds such a pair ((haplotype, pattern, pos) is unique, spm_hip.h).
// Neighbours inside [lds0, lds_end) are read from LDS, the rest from global memory (windows above the halo).
template <class Group, class GroupOf, class ScoreOf, class Allowed>
__device__ __forceinline__ bool sel_walk_keeps(const unsigned long long *s_key, const int32_t *s_score,
                                               const unsigned long long *__restrict__ keys, const sel_tile &T, long long i,
                                               Group grp, unsigned long long rel, int32_t sc, unsigned long long pos_mask,
                                               unsigned long long w, GroupOf group_of, ScoreOf score_of, Allowed allowed)
{
    for (long long j = i - 1; j >= 0; --j) { // to the left
        const bool in_lds = j >= T.lds0;
        const unsigned long long kj = in_lds ? s_key[j - T.lds0] : keys[j];
        if (group_of(kj) != grp)
            break;
        const unsigned long long rj = kj & pos_mask;
        if (rel - rj > w || !allowed(rj))
            break; // (allowed positions are one range: nothing further left is in it)
        const int32_t sj = in_lds ? s_score[j - T.lds0] : score_of(j);
        if (sj < sc || (sj == sc && rj < rel))
            return false;
    }
    for (long long j = i + 1; j < T.n; ++j) { // to the right
        const bool in_lds = j < T.lds_end;
        const unsigned long long kj = in_lds ? s_key[j - T.lds0] : keys[j];
        if (group_of(kj) != grp)
            break;
        const unsigned long long rj = kj & pos_mask;
        if (rj - rel > w || !allowed(rj))
            break;
        const int32_t sj = in_lds ? s_score[j - T.lds0] : score_of(j);
        if (sj < sc)
            return false;
    }
    return true;
}

// What the exclusive sum adds up and the compaction tests again: LOCI's verdict, and with BEST the stratum test against
// P.minima[slot_of(i)].  Params: select_params or jst_select_params, each with its sel_final(P, i) for the one functor.
template <class Params, class SlotOf>
__device__ __forceinline__ uint32_t sel_final_flag(const Params &P, uint32_t i, SlotOf slot_of)
{
    uint32_t f = P.keep[i];
    if (f && P.best)
        f = (long long)P.score[i] <= (long long)P.minima[slot_of(i)] + P.strata ? 1u : 0u;
    return f;
}
template <class Params> struct sel_flag_op
{
    Params P;
    __device__ __forceinline__ uint32_t operator()(uint32_t i) const { return sel_final(P, i); }
};

} // namespace spm_hip

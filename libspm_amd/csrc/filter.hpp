// filter.hpp -- lossless pigeonhole seed filter + bit-vector verification (dna4 texts).
//
// Why: with one lane per pattern every text byte feeds n_patterns * ~15*NW integer ops, so the brute-force scan is
// bound by the integer VALU four orders of magnitude below the HBM roof.  The reference itself
// ships the way out -- a q-gram pigeonhole filter in front of verification
// (/root/reference/libspm/libspm/matcher/pigeonhole_matcher.hpp:67-123) -- and this file is the
// MI355X formulation of that idea, arranged so that the text is streamed ONCE at HBM speed:
//
//   Pigeonhole: cut needle P (|P| = m, k errors) into k+1 disjoint seeds of q = floor(m/(k+1)) symbols.  Any
//   occurrence with <= k edits contains at least one seed unedited.  (Needles with k >= 8 get k+2 seeds: two of
//   them survive, on diagonals <= k apart -- see "candidate merging" below.)
//   Sampling:   an exact seed occurrence text[ts, ts+q) contains, for every stride S <= q-H+1, exactly one
//   H-symbol window that starts at a text position t = 0 (mod S); it equals seed[r, r+H) for r = t-ts in [0,S).
//   So it suffices to look at text windows at multiples of S and to index S shifted H-mers per seed.
//   H = 16 symbols = one 32-bit key after 2-bit packing (12..15 for seeds shorter than 17 symbols).
//
//   Level 1 (filter kernel, the streaming kernel): each lane loads 16 text bytes (one 16-byte coalesced load),
//   packs them to 2 bits/base with 4 v_dot4_u32_u8, takes the previous lane's word through DPP wave_shr:1, forms
//   the 16/S windows with v_alignbit and looks them up in a perfect-hash fingerprint table held in LDS (two LDS
//   reads per window; a Bloom cascade is kept as fallback) and records the windows that pass (survivors).  Needle
//   sets of several stride-1 passes use anchored keys: a pass looks up only the windows that begin with its dimer.
//   Resolve (resolve_kernel): survivors -> the key's entries through an exact key directory in L2 -> whole-seed and
//   piece-count checks -> diagonal bands.
//   Verification: the Myers recurrence over the m+3k symbols around the candidate diagonal, cold-started
//   m+k symbols before the first end position it is responsible for -- exact by the window property used for
//   tiling.  Short needles: one lane per candidate (verify_kernel); long needles: one lane per 32-row block
//   (verify_wave_kernel).  Duplicates (several seeds of one occurrence) are removed with an atomicCAS hash set keyed
//   by (needle, end).
//
// Exactness does not depend on the text being random: every true hit has a surviving seed, every candidate is
// verified by the full recurrence.  Pathological inputs only cost time: a span of the text that yields more survivors
// than its budget is scanned again by the brute-force kernel, that span alone.
//
// This header holds what the stages hand to each other: the survivor and band records, the growth of list chunks, the band
// table's slot format, the dedupe set.  The stages themselves, one header and one translation unit each:
//   filter_params.hpp    the kernels' parameter blocks and the constants that size their launches (no device code)
//   filter_stream.hpp    level 1: survivor chunks, the streaming skeleton, seed_filter_kernel, seed_filter_packed_kernel
//   filter_dense.hpp     the dense pass: seed_filter_dense_kernel
//   filter_resolve.hpp   resolve_kernel with its checks and queues
//   filter_verify.hpp    band selection, runs of bands, verify_kernel, verify_wave_kernel
#pragma once

#include "common.hpp"
#include "filter_shared.hpp"
#include "hd.hpp" // mix64

namespace spm_hip
{

// What the streaming kernel leaves behind: one record per text window whose key passed level 1 (practically: a real
// seed key).  The exact key table in L2 is NOT consulted while streaming -- an L2 round trip per survivor stalls a wave
// for microseconds, and a repeat-rich text has 10^7 of them; resolve_kernel looks them up afterwards, one lane per
// survivor, at full occupancy.
struct survivor
{
    uint32_t key;
    uint32_t t_lo, t_hi; // text index of the window start; t_hi == kSurvInvalid marks a reserved but unused slot
    uint32_t pad;        // pass (needle sub-batch) whose level-1 table it passed
};
constexpr uint32_t kSurvInvalid = 0xFFFFFFFFu;

// What verification works on: a band of diagonals of one needle in one haystack (segment) that collected enough seed hits.
// Bands are Bw diagonals wide, counted from `max_m` diagonals before the haystack's first symbol (so they are never
// negative); sets whose needles carry surplus seeds (k >= kMergeMinK) extend every band by k diagonals into the next one,
// so that the intact seeds of one occurrence always share a band.
struct band_rec
{
    uint32_t slot; // band table slot (seed-hit count; reset by the verification)
    uint32_t val;  // pattern << 11 | unused;  kBandInvalid marks a reserved but unused list slot
    uint32_t seg;  // segment index (0 for unsegmented scans)
    uint32_t band; // band index inside the haystack
};
constexpr uint32_t kBandInvalid = 0xFFFFFFFFu;
constexpr unsigned long long kBandEmpty = ~0ull;
static_assert(sizeof(survivor) == kSurvivorBytes && sizeof(band_rec) == kBandRecBytes, "scan_plan.hpp sizes the lists");

// Slots of the survivor and band lists are handed to the waves in chunks: one atomic on the shared counter per chunk
// instead of one per ballot (a single address takes ~100 atomics/us).  Chunks grow as a wave keeps drawing -- 32, 64, ..
// 1024 -- so a quiet text costs a few hundred wasted slots and a repeat-rich one (10^7 survivors) a few thousand atomics.
// Slots a wave reserved but did not fill are marked invalid.
// (kChunkMin = 32: scan_plan.hpp, which sizes the lists for it)
constexpr uint32_t kChunkMax = 1024;

// what one lane of the wave wrote to LDS (a queue, a chunk record) is there for the others
__device__ __forceinline__ void queue_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// The next chunk of list slots a wave draws after one of `size`: 32, 64, .. kChunkMax, and at least the n it needs now.
__device__ __forceinline__ uint32_t chunk_grow(uint32_t size, uint32_t n)
{
    const uint32_t next = size * 2 < kChunkMin ? kChunkMin : (size * 2 > kChunkMax ? kChunkMax : size * 2);
    return next < n ? n : next;
}

// Band table slot: .x = key (kBandEmpty = all ones: free), .y = value kept so that a free slot is ALL ONES (one memset
// clears the table, one 16-byte store gives a slot back): the complement of the mask of diagonals hit, or the number of
// seed hits minus one (mod 2^64).  Key and value share a slot because a table of 10^6..10^7 slots lives in HBM and a
// random access there costs a DRAM row, not bytes: the insert's compare-and-swap and the update of the value, and later
// the consumer's read and reset, touch one line each instead of two.
__device__ __forceinline__ unsigned long long band_value(unsigned long long stored, bool counting)
{
    return counting ? (unsigned long long)(uint32_t)(stored + 1ull) : ~stored;
}
__device__ __forceinline__ void band_release(ulonglong2 *tab, uint32_t slot)
{
    tab[slot] = make_ulonglong2(kBandEmpty, ~0ull);
}

// one key per reported hit in the scan's dedupe set; true if this is the first report of (pattern, end)
__device__ __forceinline__ bool seen_insert_raw(unsigned long long *seen, uint32_t seen_mask, unsigned long long *overflow,
                                                uint32_t pat, int64_t e)
{
    const unsigned long long key = ((unsigned long long)pat << 40) | (unsigned long long)e;
    uint32_t slot = (uint32_t)(mix64(key)) & seen_mask;
    // the set holds at most one key per reportable hit at load <= 1/2; a probe sequence this long means more hits than
    // it was sized for: flag it, the host starts over with a larger one
    for (uint32_t tries = 0; tries < 64; ++tries) {
        // (a set that has overflowed once is lost -- the host repeats the scan: do not grind through 64 compare-and-swaps
        // per hit of a full table, 5 s for the 46 M hits of a text with 5 % repeats)
        if (tries == 4 && __hip_atomic_load(overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)
            return false;
        const unsigned long long old = atomicCAS(&seen[slot], ~0ull, key);
        if (old == ~0ull)
            return true;
        if (old == key)
            return false;
        slot = (slot + 1) & seen_mask;
    }
    atomicAdd(overflow, 1ull);
    return false;
}

} // namespace spm_hip

// jst_reads_core.hpp -- the rule of spm_hip_jst_ref_loci_reads (contract in spm_hip.h, scheme in DESIGN.md 4.8).
// Host-compilable (g++, clang++) and device code alike: the kernels of jst_reads.hpp use the key packing and the
// classification, the CPU tests instantiate the same functions and the plain loop over them
// (tests/cpp/jst_reads_core_cases.cpp).
//
// The loci of a collapse are ordered by pattern first, so the loci of read r = pattern / strands are one contiguous run,
// forward strand before reverse, leftmost first.  The primary locus of a read is the minimum of the packed key
// (uint32) score << 32 | locus index: smallest score, then smallest index -- forward before reverse, leftmost first.
#pragma once

#include "hd.hpp"
#include "../../include/spm_hip.h"

namespace spm_hip
{

constexpr uint64_t kJstReadsNoKey = ~0ull; // the key of a read without loci (no usable locus packs to it: scores are >= 0)

SPM_HD inline uint64_t jst_reads_key(int32_t score, uint32_t locus) { return (uint64_t)(uint32_t)score << 32 | locus; }
SPM_HD inline int32_t jst_reads_key_score(uint64_t key) { return (int32_t)(uint32_t)(key >> 32); }
SPM_HD inline uint32_t jst_reads_key_locus(uint64_t key) { return (uint32_t)key; }

// strands is 1 or 2
SPM_HD inline uint32_t jst_reads_read(uint32_t pattern, uint32_t strands) { return strands == 2 ? pattern >> 1 : pattern; }
SPM_HD inline bool jst_reads_forward(uint32_t pattern, uint32_t strands) { return strands != 2 || (pattern & 1u) == 0; }

// may this locus enter the summary of n_reads reads?  (a negative score would pack above every key, the unmapped one included)
SPM_HD inline bool jst_reads_usable(uint32_t pattern, int32_t score, uint32_t strands, uint32_t n_reads)
{
    return (uint64_t)pattern < (uint64_t)strands * n_reads && score >= 0;
}

// 0: score == best, 1: score == best + 1 (in 64 bits: best may be INT32_MAX), 2: anything else
SPM_HD inline int jst_reads_class(int32_t score, int32_t best)
{
    return score == best ? 0 : (long long)score == (long long)best + 1 ? 1 : 2;
}

SPM_HD inline spm_jst_read jst_reads_unmapped(uint32_t first_locus)
{
    spm_jst_read R{};
    R.first_locus = first_locus;
    R.primary = 0xFFFFFFFFu;
    R.best = -1;
    R.best_ref_score = -1;
    return R;
}

// The whole rule as a plain loop over loci in their order: out[0 .. n_reads).  Returns the number of unusable loci; when it
// is not 0 `out` means nothing.  (The device does the same with one lane per locus: jst_reads.hpp.)
inline uint64_t jst_reads_summarise(const spm_jst_ref_locus *loci, uint64_t n, uint32_t strands, uint32_t n_reads, spm_jst_read *out)
{
    uint64_t bad = 0;
    for (uint64_t i = 0; i < n; ++i)
        bad += jst_reads_usable(loci[i].pattern, loci[i].score, strands, n_reads) ? 0 : 1;
    if (bad)
        return bad;
    uint64_t i = 0;
    for (uint32_t r = 0; r < n_reads; ++r) {
        spm_jst_read R = jst_reads_unmapped((uint32_t)i);
        uint64_t key = kJstReadsNoKey;
        const uint64_t lo = i;
        for (; i < n && jst_reads_read(loci[i].pattern, strands) == r; ++i) {
            const uint64_t k = jst_reads_key(loci[i].score, (uint32_t)i);
            key = k < key ? k : key;
            R.n_loci += 1;
            R.n_forward += jst_reads_forward(loci[i].pattern, strands) ? 1 : 0;
        }
        if (key != kJstReadsNoKey) {
            R.primary = jst_reads_key_locus(key);
            R.best = jst_reads_key_score(key);
            R.best_ref_score = loci[R.primary].ref_score;
            for (uint64_t j = lo; j < i; ++j) {
                const int c = jst_reads_class(loci[j].score, R.best);
                R.n_best += c == 0;
                R.n_next += c == 1;
            }
        }
        out[r] = R;
    }
    return 0;
}

} // namespace spm_hip

// strands.hpp -- stranded needle sets (spm_hip_patterns_create_stranded; contract in spm_hip.h, scheme in DESIGN.md 4.8): n
// reads become an ordinary set of 2n needles, pattern 2r = read r, pattern 2r + 1 = its reverse complement, both with k[r].
// Host only, plain C++17 (patterns.hip and tests/cpp/strands_cases.cpp both compile it).  Here: the complement of a rank per
// alphabet (include/libspm/seqan/alphabet.hpp has the alphabets) and build_stranded, which lays the 2n needles out for the
// ordinary create path.  Nothing downstream knows about strands: read = pattern >> 1, strand = pattern & 1 is the contract.
#pragma once

#include <cstdint>
#include <vector>

#include "../../include/spm_hip.h"

namespace spm_hip
{

// complement by rank: dna4 ACGT, dna5 ACGNT, dna15 ABCDGHKMNRSTVWY (IUPAC: B<->V, D<->H, K<->M, R<->Y; N, S, W their own)
constexpr uint8_t kComplementDna4[4] = {3, 2, 1, 0};
constexpr uint8_t kComplementDna5[5] = {4, 2, 1, 3, 0};
constexpr uint8_t kComplementDna15[15] = {11, 12, 4, 5, 2, 3, 7, 6, 8, 14, 10, 0, 1, 13, 9};

// the table of an alphabet, nullptr for a sigma that has none
inline const uint8_t *complement_table(uint32_t sigma)
{
    return sigma == 4 ? kComplementDna4 : sigma == 5 ? kComplementDna5 : sigma == 15 ? kComplementDna15 : nullptr;
}

// a rank >= sigma matches nothing on either strand: it stays what it is
inline uint8_t complement_rank(const uint8_t *table, uint32_t sigma, uint8_t r) { return r < sigma ? table[r] : r; }

struct stranded_set
{
    int status = SPM_OK;          // SPM_E_UNSUPPORTED / SPM_E_INVALID: refused, `why` says it, the vectors are empty
    const char *why = "";
    std::vector<uint8_t> ranks;   // the 2n needles back to back
    std::vector<uint32_t> offsets; // 2n + 1, from 0
    std::vector<uint16_t> k;      // 2n (empty when no k was given)
};

// ranks / offsets / k as spm_hip_patterns_create takes them (k may be null).  Both refusals for size are made from n and the
// offsets alone, before anything is allocated and before a single rank is read.
inline stranded_set build_stranded(const uint8_t *ranks, const uint32_t *offsets, uint32_t n, const uint16_t *k, uint32_t sigma)
{
    stranded_set S;
    const auto refuse = [&](int status, const char *why) {
        S.status = status;
        S.why = why;
        return S;
    };
    const uint8_t *comp = complement_table(sigma);
    if (!comp)
        return refuse(SPM_E_UNSUPPORTED, "no complement is defined for this alphabet (sigma 4, 5 and 15 have one)");
    if (2ull * n > 0xFFFFFFFFull)
        return refuse(SPM_E_UNSUPPORTED, "twice the reads do not fit a 32-bit pattern index");
    if (n && !offsets)
        return refuse(SPM_E_INVALID, "reads without offsets");
    uint64_t total = 0;
    for (uint32_t r = 0; r < n; ++r) {
        if (offsets[r + 1] < offsets[r])
            return refuse(SPM_E_INVALID, "offsets not ascending");
        total += offsets[r + 1] - offsets[r];
    }
    if (2 * total > 0xFFFFFFFFull)
        return refuse(SPM_E_UNSUPPORTED, "twice the reads' symbols do not fit a 32-bit offset");
    if (total && !ranks)
        return refuse(SPM_E_INVALID, "reads without symbols");
    S.ranks.resize(2 * total);
    S.offsets.resize(2 * (size_t)n + 1);
    if (k)
        S.k.resize(2 * (size_t)n);
    uint32_t at = 0;
    S.offsets[0] = 0;
    for (uint32_t r = 0; r < n; ++r) {
        const uint8_t *src = ranks + offsets[r];
        const uint32_t m = offsets[r + 1] - offsets[r];
        uint8_t *fwd = S.ranks.data() + at, *rev = fwd + m;
        for (uint32_t j = 0; j < m; ++j) {
            fwd[j] = src[j];
            rev[m - 1 - j] = complement_rank(comp, sigma, src[j]);
        }
        S.offsets[2 * (size_t)r + 1] = at + m;
        S.offsets[2 * (size_t)r + 2] = at + 2 * m;
        at += 2 * m;
        if (k)
            S.k[2 * (size_t)r] = S.k[2 * (size_t)r + 1] = k[r];
    }
    return S;
}

} // namespace spm_hip

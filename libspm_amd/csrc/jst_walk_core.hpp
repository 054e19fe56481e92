// jst_walk_core.hpp -- which symbols a (block, haplotype) cell of the pan-genome index owns and what its context spells
// (scheme in jst.hpp).  Host-compilable (g++, clang++) and device code alike: the build kernels of
// jst_index.hpp, the fan-outs of jst_fanout.hpp and jst_project.hpp call these functions, the CPU tests run the same ones on
// host arrays against haplotypes materialised by brute application of the allele table (tests/cpp/jst_walk_core_cases.cpp).
//   jst_alo_row        a_lo[j]: first allele with pos >= jL; the closing row n_blocks is n_alleles
//   jst_cell_delta     what the alleles of block j change in the length of haplotype h
//   jst_first_ref      first reference position at or after jL that h still reads
//   jst_hap_start      hap_start[j][h] from the exclusive column prefix of the deltas
//   jst_left_walk      the context of (j, h): where it starts, its length, its exact signature
//   jst_run_cursor     the context spelled forward as (source pointer, length) runs of the reference and of alts
#pragma once

#include <algorithm>

#include "hd.hpp"

namespace spm_hip
{

constexpr uint32_t kJstGroup = 1024;    // haplotypes whose contexts are compared with each other (signature table in LDS);
                                        // larger trees are cut into groups of this size, contexts are shared within a group
constexpr uint32_t kJstMaxHap = 65535;  // haplotype indices are reported as uint32, group-local ids are 15 bits
constexpr uint32_t kJstMaskWords = 8;   // 256 alleles per context signature; denser stretches are not shared
constexpr uint32_t kJstSigWords = 4 + kJstMaskWords;
constexpr uint16_t kJstNone = 0xFFFF;   // (block, haplotype) owns no symbol

// plain pointers: device arrays in the kernels, host arrays in the CPU tests
struct jst_dev
{
    const uint8_t *ref;
    uint64_t n_ref;
    const uint64_t *pos;
    const uint32_t *rlen, *alen;
    const uint64_t *aoff;
    const uint8_t *alt;
    const uint64_t *cov;
    uint64_t n_alleles;
    uint32_t cw, n_hap, max_rlen, window;
    uint32_t n_groups;    // ceil(n_hap / kJstGroup)
    uint64_t L, n_blocks; // all blocks of the reference
    uint64_t jb, je;      // indexed blocks
    const uint64_t *a_lo; // [n_blocks + 1]: first allele with pos >= j * L; row n_blocks = n_alleles
    uint64_t *hap_start;  // [(n_blocks + 1) * n_hap]
};

SPM_HD inline bool jst_carried(const jst_dev &J, uint64_t i, uint32_t h)
{
    return (J.cov[i * J.cw + (h >> 6)] >> (h & 63)) & 1ull;
}

SPM_HD inline uint64_t jst_alo_row(const uint64_t *pos, uint64_t n_alleles, uint64_t L, uint64_t n_blocks, uint64_t j)
{
    const uint64_t key = j * L;
    // row n_blocks closes the last block: an insertion behind the last reference symbol (pos == n_ref) belongs to it,
    // also where the block length divides n_ref and n_blocks * L == n_ref
    uint64_t lo = j == n_blocks ? n_alleles : 0, hi = n_alleles;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (pos[mid] < key)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// sum over the alleles of block j (< n_blocks) that h carries of (alt_len - ref_len)
SPM_HD inline int64_t jst_cell_delta(const jst_dev &J, uint64_t j, uint32_t h)
{
    int64_t d = 0;
    for (uint64_t i = J.a_lo[j]; i < J.a_lo[j + 1]; ++i)
        if (jst_carried(J, i, h))
            d += (int64_t)J.alen[i] - (int64_t)J.rlen[i];
    return d;
}

// first reference position at or after jL that haplotype h still reads (a carried deletion may span the block border)
SPM_HD inline uint64_t jst_first_ref(const jst_dev &J, uint64_t j, uint32_t h)
{
    const uint64_t r0 = j * J.L;
    if (j >= J.n_blocks)
        return J.n_ref;
    for (int64_t i = (int64_t)J.a_lo[j] - 1; i >= 0 && J.pos[i] + J.max_rlen > r0; --i)
        if (jst_carried(J, (uint64_t)i, h))
            return std::max<uint64_t>(r0, J.pos[i] + J.rlen[i]);
    return r0;
}

// shift = the deltas of the blocks before j summed (exclusive prefix down column h; row n_blocks holds the total)
SPM_HD inline uint64_t jst_hap_start(const jst_dev &J, uint64_t j, uint32_t h, int64_t shift)
{
    return (uint64_t)((int64_t)jst_first_ref(J, j, h) + shift);
}

// Where the context of (block j, haplotype h) starts and which alleles it spans.
struct jst_walk
{
    uint32_t sig[kJstSigWords]; // [0..1] start point, [2] first reference position - jL, [3] length, [4..] allele bits
    uint64_t start_ref;         // kind 0: reference position of the first symbol
    uint64_t start_allele;      // kind 1: allele whose alt holds the first symbol ...
    uint32_t start_off;         // ... at this offset
    uint32_t kind;              // 0 reference run, 1 inside an alt
    uint64_t next_allele;       // first allele index the forward walk examines
    uint64_t lo;                // haplotype coordinate of the first symbol
    uint32_t len, owned_from;   // context length, offset of the first owned symbol
    bool empty;                 // the cell owns nothing: only sig (all zero) is set
};

SPM_HD inline void jst_left_walk(const jst_dev &J, uint64_t j, uint32_t h, jst_walk &W)
{
    const uint64_t a = J.hap_start[j * J.n_hap + h], b = J.hap_start[(j + 1) * J.n_hap + h];
    W.empty = b <= a;
    for (uint32_t w = 0; w < kJstSigWords; ++w)
        W.sig[w] = 0;
    if (W.empty)
        return;
    const uint64_t a_hi = J.a_lo[j + 1];
    bool overflow = false;
    auto set_bit = [&](uint64_t idx) {
        const uint64_t t = a_hi - 1 - idx;
        if (t >= 32ull * kJstMaskWords) {
            overflow = true;
        } else {
            const uint32_t bit = 1u << (t & 31);
#ifdef __HIP_DEVICE_COMPILE__
#pragma unroll
#endif
            for (uint32_t w = 0; w < kJstMaskWords; ++w) // static indices: the signature stays in registers
                if ((uint32_t)(t >> 5) == w)
                    W.sig[4 + w] |= bit;
        }
    };
    for (uint64_t i = J.a_lo[j]; i < a_hi; ++i)
        if (jst_carried(J, i, h))
            set_bit(i);
    uint64_t r = jst_first_ref(J, j, h);
    const uint64_t r_first = r;
    uint64_t rem = std::min<uint64_t>(J.window ? J.window - 1 : 0, a);
    W.owned_from = (uint32_t)rem;
    W.lo = a - rem;
    W.len = (uint32_t)(rem + (b - a));
    int64_t i = (int64_t)J.a_lo[j] - 1;
    W.kind = 0;
    W.start_off = 0;
    W.start_allele = 0;
    while (true) {
        if (rem == 0) {
            W.start_ref = r;
            W.next_allele = (uint64_t)(i + 1);
            break;
        }
        while (i >= 0 && !jst_carried(J, (uint64_t)i, h))
            --i;
        if (i < 0) { // reference prefix (a >= rem guarantees r >= rem)
            W.start_ref = r - rem;
            W.next_allele = 0;
            break;
        }
        const uint64_t e = J.pos[i] + J.rlen[i];
        const uint64_t run = r - e;
        if (rem <= run) {
            W.start_ref = r - rem;
            W.next_allele = (uint64_t)(i + 1);
            break;
        }
        rem -= run;
        set_bit((uint64_t)i);
        const uint64_t al = J.alen[i];
        if (rem <= al) {
            W.kind = 1;
            W.start_allele = (uint64_t)i;
            W.start_off = (uint32_t)(al - rem);
            W.next_allele = (uint64_t)i;
            break;
        }
        rem -= al;
        r = J.pos[i];
        --i;
    }
    const uint64_t sp = W.kind ? ((1ull << 63) | (W.start_allele << 24) | W.start_off) : W.start_ref;
    W.sig[0] = (uint32_t)sp;
    W.sig[1] = (uint32_t)(sp >> 32);
    W.sig[2] = (uint32_t)(r_first - j * J.L);
    W.sig[3] = W.len;
    if (overflow) { // too many alleles for the bit set: this context is not shared
        W.sig[0] = h;
        W.sig[1] = 0xC0000000u;
    }
}

// The context of a finished (non-empty) walk W of haplotype h, spelled forward: next() yields run after run, of the
// reference or of a carried alt, n = 0 included (a deletion's alt, alleles back to back), until W.len symbols are covered.
struct jst_run_cursor
{
    uint64_t remaining, i, r; // symbols to go; the allele the walk stands at or examines next; the reference position
    uint32_t h, aoff_in;      // (aoff_in: offset inside the alt of allele i, for the first run only)
    bool in_alt;

    SPM_HD jst_run_cursor(const jst_walk &W, uint32_t h_)
        : remaining(W.len), i(W.next_allele), r(W.start_ref), h(h_), aoff_in(W.start_off), in_alt(W.kind == 1)
    {
    }
    SPM_HD bool next(const jst_dev &J, const uint8_t *&src, uint64_t &n)
    {
        if (remaining == 0 || (in_alt && i >= J.n_alleles))
            return false; // (the latter cannot happen for a validated allele table; never read past it)
        if (in_alt) {
            n = std::min<uint64_t>(remaining, (uint64_t)J.alen[i] - aoff_in);
            src = J.alt + J.aoff[i] + aoff_in;
            r = J.pos[i] + J.rlen[i];
            ++i;
            aoff_in = 0;
        } else {
            while (i < J.n_alleles && !jst_carried(J, i, h))
                ++i;
            const uint64_t run_end = i < J.n_alleles ? J.pos[i] : J.n_ref; // the last reference run ends at n_ref
            n = std::min<uint64_t>(remaining, run_end - r);
            src = J.ref + r;
            r += n;
        }
        in_alt = !in_alt; // (a reference run that did not cover the rest ended at a carried allele)
        remaining -= n;
        return true;
    }
};

} // namespace spm_hip

// jst_collapse_core.hpp -- the order and equality rule of spm_hip_jst_ref_alns_collapse (contract in spm_hip.h, scheme in
// DESIGN.md 4.6b).  Host-compilable (g++, clang++) and device code alike: the walk kernels of jst_collapse.hpp instantiate
// jst_collapse_rank with a view of the sorted slots, the CPU tests instantiate the same templates
// (tests/cpp/jst_collapse_core_cases.cpp).
//
// A locus is what a projected alignment says about the reference: needle, reference range, transcript.  Loci are ordered by
// (pattern, ref_begin, ref_end, ref_score, cigar_len) and then by their transcript words compared one by one as uint32.  The
// words decide both order and equality; no hash enters.
#pragma once

#include "hd.hpp"

namespace spm_hip
{

// what the tuple part of the order reads; the words follow it
struct jst_locus_key
{
    uint64_t ref_begin = 0, ref_end = 0;
    uint32_t pattern = 0;
    int32_t ref_score = 0;
    uint32_t cigar_len = 0;
};

template <class T> SPM_HD inline int jst_collapse_cmp3(T a, T b) { return a < b ? -1 : a > b ? 1 : 0; }

// (pattern, ref_begin, ref_end, ref_score, cigar_len), lexicographic: -1, 0, 1
SPM_HD inline int jst_collapse_cmp_tuple(const jst_locus_key &a, const jst_locus_key &b)
{
    int c = jst_collapse_cmp3(a.pattern, b.pattern);
    if (c == 0)
        c = jst_collapse_cmp3(a.ref_begin, b.ref_begin);
    if (c == 0)
        c = jst_collapse_cmp3(a.ref_end, b.ref_end);
    if (c == 0)
        c = jst_collapse_cmp3(a.ref_score, b.ref_score);
    if (c == 0)
        c = jst_collapse_cmp3(a.cigar_len, b.cigar_len);
    return c;
}

// two transcripts of n words each, word by word as uint32
SPM_HD inline int jst_collapse_cmp_words(const uint32_t *a, const uint32_t *b, uint32_t n)
{
    for (uint32_t w = 0; w < n; ++w)
        if (a[w] != b[w])
            return a[w] < b[w] ? -1 : 1;
    return 0;
}

// The whole rule.  The tuple holds cigar_len, so the words are compared only between transcripts of one length (a transcript
// that is a prefix of another is the shorter one and is decided by the tuple).
SPM_HD inline int jst_collapse_cmp(const jst_locus_key &a, const uint32_t *wa, const jst_locus_key &b, const uint32_t *wb)
{
    const int c = jst_collapse_cmp_tuple(a, b);
    return c ? c : jst_collapse_cmp_words(wa, wb, a.cigar_len);
}

struct jst_collapse_rank_result
{
    uint32_t smaller = 0;   // items of the group that are strictly smaller under the rule
    uint32_t first = 0;     // the first position of the group with equal content (self if there is none before it)
    uint32_t n_equal = 0;   // items with equal content, self included
    uint32_t n_tuple = 0;   // items with an equal tuple, self included: the run the words had to decide
};

// The in-group ranking of item `self` among the items [lo, hi) of a view V that answers key(i) and words(i).  Linear in the
// group, times the transcript length for the items whose tuple equals self's.
template <class View> SPM_HD inline jst_collapse_rank_result jst_collapse_rank(const View &V, uint32_t lo, uint32_t hi, uint32_t self)
{
    jst_collapse_rank_result R;
    R.first = self;
    const jst_locus_key k = V.key(self);
    const uint32_t *w = V.words(self);
    for (uint32_t j = lo; j < hi; ++j) {
        if (j == self) {
            ++R.n_equal;
            ++R.n_tuple;
            continue;
        }
        const jst_locus_key kj = V.key(j);
        int c = jst_collapse_cmp_tuple(kj, k);
        if (c == 0) {
            ++R.n_tuple;
            c = jst_collapse_cmp_words(V.words(j), w, k.cigar_len);
        }
        if (c < 0)
            ++R.smaller;
        else if (c == 0) {
            ++R.n_equal;
            if (j < R.first)
                R.first = j;
        }
    }
    return R;
}

// bits needed to hold the value v (0 for 0)
SPM_HD inline uint32_t jst_collapse_bits(uint64_t v)
{
    uint32_t b = 0;
    while (v) {
        ++b;
        v >>= 1;
    }
    return b;
}

// The key plan of the first sort: pattern << ref_bits | ref_begin.  ref_begin may equal the reference length (an alignment
// inside an insertion behind the last symbol), so ref_bits holds that value.
struct jst_collapse_plan
{
    uint32_t pat_bits = 0, ref_bits = 0;
    bool ok = false;
};

SPM_HD inline jst_collapse_plan plan_jst_collapse(uint32_t n_patterns, uint64_t n_ref)
{
    jst_collapse_plan p;
    p.pat_bits = jst_collapse_bits(n_patterns ? n_patterns - 1 : 0);
    p.ref_bits = jst_collapse_bits(n_ref);
    p.ok = p.pat_bits + p.ref_bits <= 64;
    return p;
}

} // namespace spm_hip

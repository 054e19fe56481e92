// jst_project_core.hpp -- projection of a pan-genome alignment onto the reference: the composition of a transcript in
// haplotype coordinates with the journal of its haplotype (contract in spm_hip.h, scheme in DESIGN.md 4.6).  Host-compilable
// (g++, clang++) and device code alike: the count and emit kernels of jst_project.hpp instantiate jst_project_compose with the
// cursor below, the CPU tests instantiate the same templates (tests/cpp/jst_project_core_cases.cpp).
//
// A journal cursor stands on one haplotype symbol and answers
//   at_end()   no symbol left
//   paired()   the symbol is paired with a reference position ...
//   rho()      ... that position; for an inserted symbol its anchor; at the end the reference length
//   next()     step to the next haplotype symbol
// A sink takes put(op, n): n columns of one op; it merges adjacent equal ops into len << 4 | op words.
#pragma once

#include "hd.hpp"

namespace spm_hip
{

constexpr uint32_t kProjIns = 1, kProjDel = 2, kProjEq = 7, kProjX = 8; // SPM_CIGAR_INS / DEL / EQ / X
constexpr uint64_t kProjMaxRun = 0x0FFFFFFFull;                         // a word holds 28 bits of length

// the allele table of a tree as plain arrays (spm_jst_allele as SoA, the coverage words)
struct jst_journal_view
{
    const uint64_t *pos = nullptr;
    const uint32_t *rlen = nullptr, *alen = nullptr;
    const uint64_t *cov = nullptr; // [n_alleles * cw]
    uint64_t n_alleles = 0;
    uint32_t cw = 0, n_hap = 0;
    uint64_t n_ref = 0;
};

// Walks the symbols of haplotype h forward from a known state: reference position r is the next one the haplotype reads,
// and no allele before table index i matters any more.  Every table index is tested against n_alleles before it is read.
struct jst_journal_cursor
{
    jst_journal_view V;
    uint32_t h = 0;
    uint64_t r = 0;       // outside an allele: the reference position of the symbol; run_end once the run is used up
    uint64_t i = 0;       // the next carried allele (n_alleles: none)
    uint64_t run_end = 0; // the run [r, run_end) is copied from the reference
    uint64_t a_pos = 0;   // inside an allele ...
    uint32_t a_rl = 0, a_al = 0, a_k = 0;
    bool in_alt = false;

    SPM_HD bool carried(uint64_t a) const { return (V.cov[a * V.cw + (h >> 6)] >> (h & 63)) & 1ull; }
    SPM_HD void find_next()
    {
        while (i < V.n_alleles && !carried(i))
            ++i;
        run_end = i < V.n_alleles ? V.pos[i] : V.n_ref;
        if (run_end < r)
            run_end = r; // (not in a validated table: a carried allele never starts inside what another one replaced)
        if (run_end > V.n_ref)
            run_end = V.n_ref;
    }
    SPM_HD void settle()
    {
        while (true) {
            if (in_alt) {
                if (a_k < a_al)
                    return;
                const uint64_t e = a_pos + a_rl;
                r = e > r ? e : r;
                in_alt = false;
                ++i;
                find_next();
            } else {
                if (r < run_end || i >= V.n_alleles)
                    return;
                a_pos = V.pos[i];
                a_rl = V.rlen[i];
                a_al = V.alen[i];
                a_k = 0;
                in_alt = true;
            }
        }
    }
    SPM_HD void start(const jst_journal_view &view, uint32_t hap, uint64_t ref_pos, uint64_t first_allele)
    {
        V = view;
        h = hap;
        r = ref_pos < view.n_ref ? ref_pos : view.n_ref;
        i = first_allele;
        in_alt = false;
        find_next();
        settle();
    }
    SPM_HD bool at_end() const { return !in_alt && r >= run_end; }
    SPM_HD bool paired() const { return !in_alt || a_k < a_rl; }
    SPM_HD uint64_t rho() const
    {
        if (!in_alt)
            return r;
        return a_pos + (a_k < a_rl ? a_k : (a_rl < a_al ? a_rl : a_al));
    }
    SPM_HD void next()
    {
        if (at_end())
            return;
        if (in_alt)
            ++a_k;
        else
            ++r;
        settle();
    }
    // n symbols forward, a run at a time; false if the haplotype ends first
    SPM_HD bool skip(uint64_t n)
    {
        while (n) {
            if (at_end())
                return false;
            if (in_alt) {
                const uint64_t t = n < (uint64_t)(a_al - a_k) ? n : (uint64_t)(a_al - a_k);
                a_k += (uint32_t)t;
                n -= t;
            } else {
                const uint64_t t = n < run_end - r ? n : run_end - r;
                r += t;
                n -= t;
            }
            settle();
        }
        return true;
    }
};

// the run merger of both sinks: word(w) is the only thing they differ in
template <class Derived>
struct jst_proj_sink_base
{
    uint32_t op = 0;
    uint64_t len = 0, n_words = 0;
    SPM_HD void flush()
    {
        while (len) {
            const uint64_t t = len < kProjMaxRun ? len : kProjMaxRun;
            static_cast<Derived *>(this)->word((uint32_t)(t << 4) | op);
            ++n_words;
            len -= t;
        }
    }
    SPM_HD void put(uint32_t o, uint64_t n)
    {
        if (n == 0)
            return;
        if (o != op) {
            flush();
            op = o;
        }
        len += n;
    }
};

struct jst_proj_count_sink : jst_proj_sink_base<jst_proj_count_sink>
{
    SPM_HD void word(uint32_t) {}
};

struct jst_proj_write_sink : jst_proj_sink_base<jst_proj_write_sink>
{
    uint32_t *out = nullptr;
    uint64_t cap = 0; // words the slot holds: nothing is written beyond them
    SPM_HD void word(uint32_t w)
    {
        if (n_words < cap)
            out[n_words] = w;
    }
};

struct jst_proj_result
{
    uint64_t ref_begin = 0, ref_end = 0;
    uint64_t n_words = 0;
    uint64_t ref_score = 0; // X + I + D symbols of the projected transcript
    uint32_t inside = 0;    // 1: no column consumes a reference position (the alignment lies inside one inserted stretch)
};

// The projection of (transcript words[0, n_words) of `needle` against the haplotype symbols from where J stands) through the
// journal J walks.  ref[0, n_ref) are the reference's ranks; = / X compare ranks.  false: the input is not what the contract
// promises (an unknown op, a transcript that consumes more or less than the needle or more than the haplotype, a reference
// position that does not grow or lies outside the reference); R and the sink are then not to be used.
template <class Cursor, class Sink>
SPM_HD inline bool jst_project_compose(Cursor &J, const uint32_t *words, uint32_t n_words, const uint8_t *needle, uint32_t m,
                                       const uint8_t *ref, uint64_t n_ref, Sink &S, jst_proj_result &R)
{
    const uint64_t anchor = J.rho();
    bool have = false;
    uint64_t prev = 0, first = 0, score = 0;
    uint32_t i = 0;
    for (uint32_t w = 0; w < n_words; ++w) {
        const uint32_t op = words[w] & 15u;
        const uint32_t len = words[w] >> 4;
        if (op == kProjIns) {
            if (len > m - i)
                return false;
            S.put(kProjIns, len);
            score += len;
            i += len;
            continue;
        }
        if (op != kProjEq && op != kProjX && op != kProjDel)
            return false;
        const bool del = op == kProjDel;
        for (uint32_t c = 0; c < len; ++c) {
            if (J.at_end() || (!del && i >= m))
                return false;
            if (J.paired()) {
                const uint64_t rho = J.rho();
                if (rho >= n_ref || (have && rho <= prev))
                    return false;
                if (have) {
                    S.put(kProjDel, rho - prev - 1); // what a carried allele deleted between the two
                    score += rho - prev - 1;
                } else {
                    first = rho;
                }
                have = true;
                prev = rho;
                if (del) {
                    S.put(kProjDel, 1);
                    ++score;
                } else {
                    const bool eq = needle[i] == ref[rho];
                    S.put(eq ? kProjEq : kProjX, 1);
                    score += eq ? 0 : 1;
                    ++i;
                }
            } else if (!del) {
                S.put(kProjIns, 1);
                ++score;
                ++i;
            }
            J.next();
        }
    }
    S.flush();
    R.ref_begin = have ? first : anchor;
    R.ref_end = have ? prev + 1 : anchor;
    R.n_words = S.n_words;
    R.ref_score = score;
    R.inside = have ? 0u : 1u;
    return i == m;
}

} // namespace spm_hip

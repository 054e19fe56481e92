// select_plan.hpp -- what one hit selection (spm_hip_hits_select / spm_hip_records_select) decides on the host, as pure
// functions (plain C++17, no HIP: select.hip and tests/cpp/select_plan_cases.cpp both compile it): the window a needle
// gets, the bit budget of the sort key, the halo the selection kernel stages in LDS, and the two refusals that are made
// before anything is launched (SPM_SELECT_STRANDS: the flag needs BEST, the minima table is per read).  select.hip keeps the
// HIP calls and acts on the answers.  Also here: plan_jst_select for
// pan-genome selections (front and back shared with plan_select) and plan_jst_locate for spm_hip_jst_selection_align's sort.
#pragma once

#include <algorithm>
#include <cstdint>

#include "../../include/spm_hip.h"

namespace spm_hip
{

constexpr uint32_t kSelTile = 256;    // records per workgroup of select_loci_kernel (one lane each)
constexpr uint32_t kSelHaloCap = 32;  // records staged in LDS on either side of a tile, at most

// bits needed to hold v: 0 for 0, 1 for 1, 2 for 2..3, ... 64 for v >= 2^63
inline uint32_t bits_for(uint64_t v)
{
    uint32_t b = 0;
    while (v) {
        ++b;
        v >>= 1;
    }
    return b;
}

// The window of one needle.  SPM_SELECT_WINDOW_K: the needle's own k -- 0 for exact sets, whose k the matchers ignore.
inline uint32_t select_window(uint32_t opt_window, bool myers_set, uint32_t k)
{
    if (opt_window != SPM_SELECT_WINDOW_K)
        return opt_window;
    return myers_set ? k : 0u;
}

// Records of one pattern have distinct positions, so at most `window` neighbours on either side lie inside the window:
// that many are staged beside the tile, up to the cap (beyond it the kernel reads global memory).
inline uint32_t select_halo(uint32_t max_window, uint32_t cap = kSelHaloCap) { return std::min(max_window, cap); }

struct select_plan
{
    int status = SPM_OK;       // SPM_E_UNSUPPORTED / SPM_E_INVALID: refused, `why` says it
    const char *why = "";
    uint32_t pat_bits = 0;     // key = pattern << pos_bits | (pos - bias)
    uint32_t pos_bits = 0;
    uint32_t key_bits = 0;     // the radix sort's end_bit
    uint32_t window = 0;       // the one window of every needle, or SPM_SELECT_WINDOW_K: read k per needle on the device
    uint32_t max_window = 0;   // the largest window any needle gets
    uint32_t halo = 0;
    bool loci = false, best = false;
    bool strands = false;      // SPM_SELECT_STRANDS: BEST's minimum is per read = pattern >> 1
    uint64_t min_slots = 0;    // entries of the minima table BEST needs (0 without BEST)
};

// a refusal: status and why are set, and nothing else of P means anything
template <class Plan> bool plan_refuse(Plan &P, int status, const char *why)
{
    P.status = status;
    P.why = why;
    return false;
}

// The front that every selection plan shares: the flag bits (`allowed`: the flags this kind of selection takes), what
// the flags need, and the record count.  False: refused.
template <class Plan> bool plan_select_front(Plan &P, const spm_select_opts &o, uint32_t allowed, uint64_t n_records, bool have_k)
{
    if ((o.flags & ~allowed) || o.reserved)
        return plan_refuse(P, SPM_E_INVALID, "unknown flag bits, or a nonzero reserved field");
    P.loci = (o.flags & SPM_SELECT_LOCI) != 0;
    P.best = (o.flags & SPM_SELECT_BEST) != 0;
    if ((o.flags & SPM_SELECT_ACROSS) && !P.best)
        return plan_refuse(P, SPM_E_INVALID, "SPM_SELECT_ACROSS needs SPM_SELECT_BEST");
    P.strands = (o.flags & SPM_SELECT_STRANDS) != 0;
    if (P.strands && !P.best)
        return plan_refuse(P, SPM_E_INVALID, "SPM_SELECT_STRANDS needs SPM_SELECT_BEST");
    if (P.loci && o.window == SPM_SELECT_WINDOW_K && !have_k)
        return plan_refuse(P, SPM_E_INVALID, "SPM_SELECT_WINDOW_K needs the needle set");
    if (n_records > 0xFFFFFFFFull)
        return plan_refuse(P, SPM_E_UNSUPPORTED, "more than 2^32 - 1 records");
    return true;
}

// Entries of a minima table indexed by pattern, or under SPM_SELECT_STRANDS by read = pattern >> 1: the patterns
// 0 .. n_patterns - 1 name the reads 0 .. (n_patterns - 1) >> 1.
inline uint64_t select_minima_slots(uint64_t n_patterns, bool strands)
{
    const uint64_t n = std::max<uint64_t>(n_patterns, 1);
    return strands ? ((n - 1) >> 1) + 1 : n;
}

// ... and the back, once the key's fields are sized: above 64 bits refused with `too_wide`; the window(s) and the halo
template <class Plan>
void plan_select_back(Plan &P, const spm_select_opts &o, bool myers_set, uint32_t max_k, const char *too_wide)
{
    if (P.key_bits > 64) {
        plan_refuse(P, SPM_E_UNSUPPORTED, too_wide);
        return;
    }
    P.key_bits = std::max(P.key_bits, 1u);
    if (P.loci) {
        const bool per_needle = o.window == SPM_SELECT_WINDOW_K && myers_set && max_k > 0;
        P.window = per_needle ? SPM_SELECT_WINDOW_K : select_window(o.window, myers_set, max_k);
        P.max_window = select_window(o.window, myers_set, max_k);
    }
    P.halo = select_halo(P.max_window);
}

// n_records: records to select from; n_patterns: patterns the records can name (>= 1); max_rel_pos: the largest
// pos - bias a record can hold; myers_set / have_k / max_k: the needle set (have_k false: no set was given).
inline select_plan plan_select(const spm_select_opts &o, uint64_t n_records, uint64_t n_patterns, uint64_t max_rel_pos,
                               bool have_k, bool myers_set, uint32_t max_k)
{
    select_plan P;
    if (!plan_select_front(P, o, SPM_SELECT_LOCI | SPM_SELECT_BEST | SPM_SELECT_STRANDS, n_records, have_k))
        return P;
    P.min_slots = P.best ? select_minima_slots(n_patterns, P.strands) : 0;
    P.pat_bits = bits_for(n_patterns ? n_patterns - 1 : 0);
    P.pos_bits = bits_for(max_rel_pos);
    P.key_bits = P.pat_bits + P.pos_bits;
    plan_select_back(P, o, myers_set, max_k, "pattern index and position do not fit one 64-bit sort key");
    return P;
}

// ---- pan-genome selections (spm_hip_jst_hits_select / spm_hip_jst_records_select; jst_select.hip) -------------------------
// The locus of a spm_jst_hit is (haplotype, pattern): key = haplotype << (pat_bits + pos_bits) | pattern << pos_bits | pos,
// so key >> pos_bits names the group whose records see each other.  Positions are haplotype coordinates from 0: no bias.
struct jst_select_plan
{
    int status = SPM_OK;
    const char *why = "";
    uint32_t hap_bits = 0, pat_bits = 0, pos_bits = 0;
    uint32_t key_bits = 0;     // the radix sort's end_bit (>= 1)
    uint32_t window = 0;       // as select_plan
    uint32_t max_window = 0;
    uint32_t halo = 0;
    bool loci = false, best = false, across = false;
    bool strands = false;      // SPM_SELECT_STRANDS: the minimum's group is (haplotype, read), or with ACROSS the read
    uint64_t min_slots = 0;    // entries of the minima table: per read or pattern with ACROSS, else one per record at most
};

// n_haplotypes / n_patterns: what the records can name (>= 1 each); max_pos: the largest position a record can hold (for a
// tree: reference length plus all inserted symbols); the needle set as in plan_select.
inline jst_select_plan plan_jst_select(const spm_select_opts &o, uint64_t n_records, uint64_t n_haplotypes, uint64_t n_patterns,
                                       uint64_t max_pos, bool have_k, bool myers_set, uint32_t max_k)
{
    jst_select_plan P;
    if (!plan_select_front(P, o, SPM_SELECT_LOCI | SPM_SELECT_BEST | SPM_SELECT_ACROSS | SPM_SELECT_STRANDS, n_records, have_k))
        return P;
    P.across = (o.flags & SPM_SELECT_ACROSS) != 0;
    P.min_slots = !P.best ? 0 : P.across ? select_minima_slots(n_patterns, P.strands) : n_records;
    P.hap_bits = bits_for(n_haplotypes ? n_haplotypes - 1 : 0);
    P.pat_bits = bits_for(n_patterns ? n_patterns - 1 : 0);
    if (P.strands) // the strand is the lowest bit of the group: it must be a pattern bit even where only pattern 0 occurs
        P.pat_bits = std::max(P.pat_bits, 1u);
    P.pos_bits = bits_for(max_pos);
    P.key_bits = P.hap_bits + P.pat_bits + P.pos_bits;
    plan_select_back(P, o, myers_set, max_k, "haplotype, pattern index and position do not fit one 64-bit sort key");
    return P;
}

// ---- spm_hip_jst_selection_align: the kept records of a pan-genome selection are ordered by the segment hit they map to,
// key = pattern << ctx_bits | position in the context buffer (positions run up to ctx_symbols inclusive: an exclusive end).
struct jst_locate_plan
{
    int status = SPM_OK;
    const char *why = "";
    uint32_t pat_bits = 0, ctx_bits = 0;
    uint32_t key_bits = 0; // what the radix sort looks at (at least 1)
};

inline jst_locate_plan plan_jst_locate(uint64_t n_records, uint64_t n_patterns, uint64_t ctx_symbols)
{
    jst_locate_plan P;
    P.pat_bits = bits_for(n_patterns ? n_patterns - 1 : 0);
    P.ctx_bits = bits_for(ctx_symbols);
    if (n_records > 0xFFFFFFFFull) {
        plan_refuse(P, SPM_E_UNSUPPORTED, "more than 2^32 - 1 records");
        return P;
    }
    if (P.pat_bits + P.ctx_bits > 64) {
        plan_refuse(P, SPM_E_UNSUPPORTED, "pattern index and context position do not fit a 64-bit sort key");
        return P;
    }
    P.key_bits = std::max(1u, P.pat_bits + P.ctx_bits);
    return P;
}

} // namespace spm_hip

// jst_rescue_core.hpp -- the rule of spm_hip_jst_pairs_rescue (contract in spm_hip.h, scheme in DESIGN.md 4.10).
// Host-compilable (g++, clang++) and device code alike: the kernels of jst_rescue.hpp use the job derivation, the window, the
// chunk geometry, the bit-vector column, the chunk scan, the key packing and the record; the CPU tests instantiate the same
// functions (tests/cpp/jst_rescue_core_cases.cpp).
//
// A pair without a proper combination gives one job per mapped mate: the anchor A is the locus the pair record reports for
// that mate, and the job looks for the OTHER mate on the opposite strand inside the stretch of the reference the fragment
// bounds allow, with up to k edits.  The search is semi-global unit-cost edit distance (Myers' bit-vector recurrence, NW
// 64-bit words), the candidate the minimum of (distance, end) over the admissible ends.
#pragma once

#include "hd.hpp"
#include "jst_pairs_core.hpp"

namespace spm_hip
{

constexpr uint64_t kJstRescueNoKey = ~0ull; // no admissible end within k
constexpr uint32_t kJstRescueLanes = 64;    // the end range of a job is cut into this many chunks
constexpr uint32_t kJstRescueMaxM = 256;    // four 64-bit words

SPM_HD inline bool jst_rescue_opts_ok(const spm_jst_rescue_opts &o)
{
    return o.flags == 0 && o.reserved == 0 && o.min_tlen >= 1 && o.min_tlen <= o.max_tlen && o.max_tlen <= 0x7FFFFFFFu;
}

// the needle of a job: the other mate of the anchor's read, on the opposite strand
SPM_HD inline uint32_t jst_rescue_needle(uint32_t pair, uint32_t anchor_mate, uint32_t anchor_pattern)
{
    return 4u * pair + 2u * (anchor_mate ^ 1u) + (1u - (anchor_pattern & 1u));
}

// Which mates of a pair record anchor a job: bit 0 mate 1 (it rescues mate 2), bit 1 mate 2 (it rescues mate 1).  Jobs are
// ordered by the mate they RESCUE: the job anchored at mate 2 comes first.
SPM_HD inline uint32_t jst_rescue_anchors(const spm_jst_pair &R)
{
    if (R.flag1 & 0x2u)
        return 0;
    return (R.locus1 != kJstPairsNone ? 1u : 0u) | (R.locus2 != kJstPairsNone ? 2u : 0u);
}
SPM_HD inline uint32_t jst_rescue_job_count(uint32_t anchors) { return (anchors & 1u) + (anchors >> 1); }

// Does the pair record agree with the read summary, the loci and the reference?  Every index is tested before it is one.
SPM_HD inline bool jst_rescue_pair_ok(const spm_jst_ref_locus *loci, uint64_t n, const spm_jst_read &M1, const spm_jst_read &M2,
                                      const spm_jst_pair &R, uint32_t pair, uint64_t N)
{
    const uint32_t locus[2] = {R.locus1, R.locus2};
    const uint16_t flag[2] = {R.flag1, R.flag2};
    const uint32_t primary[2] = {M1.primary, M2.primary};
    if (((R.flag1 ^ R.flag2) & 0x2u) != 0)
        return false;
    for (uint32_t x = 0; x < 2; ++x) {
        const bool un = locus[x] == kJstPairsNone;
        if (un != ((flag[x] & 0x4u) != 0) || un != ((flag[x ^ 1u] & 0x8u) != 0))
            return false;
        if (un)
            continue;
        if (locus[x] >= n)
            return false;
        const spm_jst_ref_locus &A = loci[locus[x]];
        if ((A.pattern >> 1) != 2u * pair + x || ((A.pattern & 1u) != 0) != ((flag[x] & 0x10u) != 0))
            return false;
        if (A.ref_begin > A.ref_end || A.ref_end > N)
            return false;
        if (!(R.flag1 & 0x2u) && locus[x] != primary[x]) // (a pair that is not proper reports the read summary's primaries)
            return false;
    }
    return true;
}

// the stretch of the reference a job searches, and the exclusive ends a candidate may have: [e_first, e_first + n_ends)
struct jst_rescue_window
{
    uint64_t lo = 0, hi = 0;  // window [lo, hi): no alignment begins left of lo
    uint64_t e_first = 0;
    uint32_t n_ends = 0;      // 0: nothing can be found
};

SPM_HD inline jst_rescue_window jst_rescue_window_of(uint64_t a_begin, uint64_t a_end, bool a_reverse, uint32_t min_tlen,
                                                     uint32_t max_tlen, uint64_t N)
{
    jst_rescue_window W;
    uint64_t e_last;
    if (!a_reverse) {
        W.lo = a_begin;
        W.hi = N - a_begin < max_tlen ? N : a_begin + max_tlen; // (a_begin <= a_end <= N)
        const uint64_t least = N - a_begin < min_tlen ? N + 1 : a_begin + min_tlen;
        W.e_first = least > a_end ? least : a_end;
        e_last = W.hi;
    } else {
        W.lo = a_end > max_tlen ? a_end - max_tlen : 0;
        W.hi = a_end;
        W.e_first = W.lo + 1;
        e_last = a_end;
    }
    W.n_ends = e_last >= W.e_first ? (uint32_t)(e_last - W.e_first + 1) : 0u; // (at most max_tlen + 1 <= 2^31)
    return W;
}

// chunk i of 64: its ends [first, first + len) and the text position its scan starts cold at.  The first n_ends mod 64
// chunks hold one end more; a chunk without an end idles.
struct jst_rescue_chunk
{
    uint64_t first = 0, start = 0;
    uint32_t len = 0;
};

SPM_HD inline jst_rescue_chunk jst_rescue_chunk_of(const jst_rescue_window &W, uint32_t i, uint32_t m, uint32_t k)
{
    jst_rescue_chunk C;
    const uint32_t q = W.n_ends / kJstRescueLanes, r = W.n_ends % kJstRescueLanes;
    C.len = q + (i < r ? 1u : 0u);
    C.first = W.e_first + (uint64_t)i * q + (i < r ? i : r);
    const uint64_t back = 1ull + m + k;
    C.start = C.first - W.lo > back ? C.first - back : W.lo; // (first > lo: ends are exclusive and an end of lo is never admissible)
    return C;
}

SPM_HD inline uint64_t jst_rescue_key(uint32_t d, uint64_t rel_end) { return (uint64_t)d << 32 | (uint32_t)rel_end; }
SPM_HD inline uint32_t jst_rescue_key_d(uint64_t key) { return (uint32_t)(key >> 32); }
SPM_HD inline uint32_t jst_rescue_key_rel(uint64_t key) { return (uint32_t)key; }

// the forward match masks of a needle: masks[c * NW + w] bit i: symbol 64 w + i has rank c.  A rank >= sigma sets no bit.
inline void jst_rescue_masks(const uint8_t *needle, uint32_t m, uint32_t sigma, uint32_t NW, uint64_t *masks)
{
    for (uint32_t j = 0; j < sigma * NW; ++j)
        masks[j] = 0;
    for (uint32_t i = 0; i < m; ++i)
        if (needle[i] < sigma)
            masks[needle[i] * NW + i / 64] |= 1ull << (i % 64);
}

// one 64-bit block of Myers' recurrence with the horizontal delta hin (-1, 0, +1) coming in from the block above; returns
// the delta going out of its last row.  ph / mh: bit r says row r of the block rose / fell by one in this column.
SPM_HD inline int jst_rescue_block(uint64_t &pv, uint64_t &mv, uint64_t eq, int hin, uint64_t &ph_out, uint64_t &mh_out)
{
    const uint64_t neg = hin < 0 ? 1ull : 0ull;
    const uint64_t xv = eq | mv;
    eq |= neg;
    const uint64_t xh = (((eq & pv) + pv) ^ pv) | eq;
    uint64_t ph = mv | ~(xh | pv);
    uint64_t mh = pv & xh;
    ph_out = ph;
    mh_out = mh;
    const int hout = (int)(ph >> 63) - (int)(mh >> 63);
    ph = (ph << 1) | (hin > 0 ? 1ull : 0ull);
    mh = (mh << 1) | neg;
    pv = mh | ~(xv | ph);
    mv = ph & xv;
    return hout;
}

// One chunk: the semi-global scan of text[start ..) up to the chunk's last end, cold (every begin costs nothing), and the
// minimal key over the chunk's ends whose distance is <= k.  start >= lo and start <= first - 1 - (m + k) or start == lo: an
// alignment with at most k edits that ends at e spans at most m + k symbols, so inside the chunk every distance <= k is the
// distance of the whole window and none is missed.  masks: [sigma][NW]; a text rank >= sigma matches nothing.
template <int NW>
SPM_HD inline uint64_t jst_rescue_chunk_scan(const uint64_t *masks, uint32_t sigma, uint32_t m, uint32_t k, const uint8_t *text,
                                             const jst_rescue_chunk &C, uint64_t lo)
{
    uint64_t best = kJstRescueNoKey;
    if (C.len == 0)
        return best;
    uint64_t pv[NW], mv[NW];
#ifdef __HIP_DEVICE_COMPILE__
#pragma unroll
#endif
    for (int w = 0; w < NW; ++w) {
        pv[w] = ~0ull;
        mv[w] = 0;
    }
    const uint32_t lb = (m - 1) & 63;
    uint32_t score = m;
    const uint64_t last = C.first + C.len - 1; // the chunk's last end: the scan reads text[start .. last - 1]
    for (uint64_t t = C.start; t < last; ++t) {
        const uint32_t c = text[t];
        const uint64_t *eq = masks + (size_t)(c < sigma ? c : 0u) * NW;
        const uint64_t live = c < sigma ? ~0ull : 0ull;
        int h = 0;
        uint64_t ph = 0, mh = 0;
#ifdef __HIP_DEVICE_COMPILE__
#pragma unroll
#endif
        for (int w = 0; w < NW; ++w)
            h = jst_rescue_block(pv[w], mv[w], eq[w] & live, h, ph, mh);
        score += (uint32_t)((ph >> lb) & 1) - (uint32_t)((mh >> lb) & 1);
        const uint64_t e = t + 1;
        if (e >= C.first && score <= k) {
            const uint64_t key = jst_rescue_key(score, e - lo);
            best = key < best ? key : best;
        }
    }
    return best;
}

// the whole search of one job as a plain loop over the 64 chunks (the device gives each chunk a lane and takes the minimum
// with shuffles)
template <int NW>
inline uint64_t jst_rescue_search(const uint64_t *masks, uint32_t sigma, uint32_t m, uint32_t k, const uint8_t *text,
                                  const jst_rescue_window &W)
{
    uint64_t best = kJstRescueNoKey;
    for (uint32_t i = 0; i < kJstRescueLanes; ++i) {
        const uint64_t key = jst_rescue_chunk_scan<NW>(masks, sigma, m, k, text, jst_rescue_chunk_of(W, i, m, k), W.lo);
        best = key < best ? key : best;
    }
    return best;
}

// The record of one job.  A: the anchor; anchor_mate: 0 when it is mate 1's.  found: the search had a candidate, whose
// alignment is [begin, end) with `score` edits.  The concordance of (anchor, rescued alignment) is tested post hoc with
// the predicate of the pairing; a candidate that fails it keeps its alignment (NOT_CONCORDANT), and no other end is tried.
SPM_HD inline spm_jst_rescue jst_rescue_record(const spm_jst_ref_locus &A, uint32_t anchor, uint32_t pair, uint32_t anchor_mate,
                                               uint32_t pattern, bool found, uint64_t begin, uint64_t end, int32_t score,
                                               uint32_t cigar_off, uint32_t cigar_len, uint32_t min_tlen, uint32_t max_tlen)
{
    spm_jst_rescue O{};
    O.pair = pair;
    O.pattern = pattern;
    O.anchor = anchor;
    O.score = -1;
    O.status = SPM_RESCUE_NONE;
    const bool a_reverse = (A.pattern & 1u) != 0, mate2 = anchor_mate == 0;
    if (found) {
        spm_jst_ref_locus Y{};
        Y.ref_begin = begin;
        Y.ref_end = end;
        const bool ok = a_reverse ? jst_pairs_concordant(Y, A, min_tlen, max_tlen) : jst_pairs_concordant(A, Y, min_tlen, max_tlen);
        O.ref_begin = begin;
        O.ref_end = end;
        O.score = score;
        O.cigar_off = cigar_off;
        O.cigar_len = cigar_len;
        O.status = ok ? SPM_RESCUE_RESCUED : SPM_RESCUE_NOT_CONCORDANT;
        if (ok) {
            const int32_t t = (int32_t)(a_reverse ? A.ref_end - begin : end - A.ref_begin);
            const bool mate1_forward = a_reverse ? mate2 == false : anchor_mate == 0;
            O.tlen = mate1_forward ? t : -t;
        }
    }
    O.flag = jst_pairs_flag(mate2, O.status == SPM_RESCUE_RESCUED, !found, false, found && !a_reverse, a_reverse);
    return O;
}

} // namespace spm_hip

// jst_pairs_core.hpp -- the rule of spm_hip_jst_ref_loci_pairs (contract in spm_hip.h, scheme in DESIGN.md 4.9).
// Host-compilable (g++, clang++) and device code alike: the kernels of jst_pairs.hpp use the concordance test, the walk of a
// partner window, the key packing and the record; the CPU tests instantiate the same functions and the plain loop over them
// (tests/cpp/jst_pairs_core_cases.cpp).
//
// Reads 2p and 2p + 1 of a stranded set are the mates of pair p, so the loci of pair p are the contiguous patterns
// 4p (mate 1 forward), 4p + 1 (mate 1 reverse), 4p + 2 (mate 2 forward), 4p + 3 (mate 2 reverse), each sub-run ascending in
// ref_begin.  A forward locus a and a reverse locus b of the OTHER mate are concordant iff a lies left of b and the fragment
// [a.ref_begin, b.ref_end) has an allowed length.  The best pair is the minimum of (a.score + b.score, a, b): for a fixed a the
// best partner is the minimum of (b.score, b), and the pair's key is (uint32) sum << 32 | a.
#pragma once

#include "hd.hpp"
#include "../../include/spm_hip.h"

namespace spm_hip
{

constexpr uint64_t kJstPairsNoKey = ~0ull;     // the key of a pair without a concordant combination (sums are < 2^31)
constexpr uint32_t kJstPairsNone = 0xFFFFFFFFu; // no locus, no partner

SPM_HD inline bool jst_pairs_opts_ok(const spm_jst_pair_opts &o)
{
    return o.flags == 0 && o.reserved == 0 && o.min_tlen >= 1 && o.min_tlen <= o.max_tlen && o.max_tlen <= 0x7FFFFFFFu;
}

SPM_HD inline uint32_t jst_pairs_pair(uint32_t pattern) { return pattern >> 2; }
SPM_HD inline bool jst_pairs_reverse(uint32_t pattern) { return (pattern & 1u) != 0; }
SPM_HD inline bool jst_pairs_mate2(uint32_t pattern) { return (pattern & 2u) != 0; }

SPM_HD inline uint64_t jst_pairs_key(uint32_t sum, uint32_t a) { return (uint64_t)sum << 32 | a; }
SPM_HD inline uint32_t jst_pairs_key_sum(uint64_t key) { return (uint32_t)(key >> 32); }
SPM_HD inline uint32_t jst_pairs_key_a(uint64_t key) { return (uint32_t)key; }

// forward locus a of one mate, reverse locus b of the other
SPM_HD inline bool jst_pairs_concordant(const spm_jst_ref_locus &a, const spm_jst_ref_locus &b, uint32_t min_tlen, uint32_t max_tlen)
{
    if (a.ref_begin > b.ref_begin || a.ref_end > b.ref_end || b.ref_end < a.ref_begin)
        return false;
    const uint64_t t = b.ref_end - a.ref_begin;
    return t >= min_tlen && t <= max_tlen;
}

// the score sum of a combination, in 64 bits; false: it does not fit in 31 bits (or a score is negative) -- unusable
SPM_HD inline bool jst_pairs_sum(int32_t score_a, int32_t score_b, uint32_t &sum)
{
    const long long s = (long long)score_a + (long long)score_b;
    if (score_a < 0 || score_b < 0 || s > 0x7FFFFFFFll)
        return false;
    sum = (uint32_t)s;
    return true;
}

SPM_HD inline uint32_t jst_pairs_clamp(uint64_t x) { return x > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)x; }

// Does the record of `read` agree with n loci?  Everything the rule uses as an index is tested here before it is one: the run
// lies inside the loci, the patterns at the head and the tail of both sub-runs name the read and its strand, the primary lies
// inside the run.  (reads are < 2^31: the summary was made with strands == 2.)
SPM_HD inline bool jst_pairs_read_ok(const spm_jst_ref_locus *loci, uint64_t n, const spm_jst_read &R, uint32_t read)
{
    if (R.n_forward > R.n_loci || (uint64_t)R.first_locus + R.n_loci > n)
        return false;
    if (R.n_loci == 0)
        return R.primary == kJstPairsNone;
    const uint32_t lo = R.first_locus, mid = lo + R.n_forward, hi = lo + R.n_loci;
    const uint64_t fwd = 2ull * read, rev = fwd + 1;
    if (loci[lo].pattern != (R.n_forward ? fwd : rev) || loci[hi - 1].pattern != (mid < hi ? rev : fwd))
        return false;
    if (R.n_forward && loci[mid - 1].pattern != fwd)
        return false;
    if (mid < hi && loci[mid].pattern != rev)
        return false;
    return R.primary >= lo && R.primary < hi;
}

// Does the record R of locus i's own read hold i, on the side its pattern names?
SPM_HD inline bool jst_pairs_covers(const spm_jst_read &R, uint64_t n, uint32_t i, uint32_t pattern)
{
    if (R.n_forward > R.n_loci || (uint64_t)R.first_locus + R.n_loci > n || i < R.first_locus || i - R.first_locus >= R.n_loci)
        return false;
    return (i - R.first_locus < R.n_forward) != jst_pairs_reverse(pattern);
}

struct jst_pairs_walked
{
    uint32_t partner = kJstPairsNone; // the concordant b with the smallest (score, index)
    uint32_t sum = 0;                 // a.score + partner.score
    uint32_t window = 0;              // loci walked
    uint64_t n_pairs = 0, n_best = 0, n_next = 0;
    uint64_t unusable = 0;            // concordant combinations whose sum does not fit
};

// One forward locus a against [lo, hi), the reverse run of the other mate (ascending in ref_begin): the window of
// b.ref_begin in [a.ref_begin, a.ref_begin + max_tlen] by a lower bound -- a necessary condition -- and the rest of the rule
// on every b inside.  target: the pair's best sum, for n_best / n_next; -1 while it is not known.
SPM_HD inline jst_pairs_walked jst_pairs_walk(const spm_jst_ref_locus *loci, uint32_t a, uint32_t lo, uint32_t hi, uint32_t min_tlen,
                                              uint32_t max_tlen, long long target)
{
    jst_pairs_walked W;
    const spm_jst_ref_locus A = loci[a];
    const uint64_t last = A.ref_begin > ~0ull - max_tlen ? ~0ull : A.ref_begin + max_tlen;
    uint32_t l = lo, h = hi;
    while (l < h) {
        const uint32_t mid = l + (h - l) / 2;
        if (loci[mid].ref_begin < A.ref_begin)
            l = mid + 1;
        else
            h = mid;
    }
    int32_t partner_score = 0;
    for (uint32_t b = l; b < hi && loci[b].ref_begin <= last; ++b) {
        W.window += 1;
        const spm_jst_ref_locus B = loci[b];
        if (!jst_pairs_concordant(A, B, min_tlen, max_tlen))
            continue;
        uint32_t sum;
        if (!jst_pairs_sum(A.score, B.score, sum)) {
            W.unusable += 1;
            continue;
        }
        W.n_pairs += 1;
        W.n_best += (long long)sum == target;
        W.n_next += (long long)sum == target + 1 && target >= 0;
        if (W.partner == kJstPairsNone || B.score < partner_score) { // (ascending b: the first of equal scores stays)
            W.partner = b;
            partner_score = B.score;
            W.sum = sum;
        }
    }
    return W;
}

SPM_HD inline uint16_t jst_pairs_flag(bool mate2, bool proper, bool self_unmapped, bool other_unmapped, bool self_reverse,
                                      bool other_reverse)
{
    return (uint16_t)(0x1u | (proper ? 0x2u : 0u) | (self_unmapped ? 0x4u : 0u) | (other_unmapped ? 0x8u : 0u) |
                      (self_reverse ? 0x10u : 0u) | (other_reverse ? 0x20u : 0u) | (mate2 ? 0x80u : 0x40u));
}

// The record of one pair.  key: the pair's minimal key, b: partner[a] of its a (both are loci indices below the loci
// count); primary1 / primary2: the mates' own primaries, reported when no combination is concordant.
SPM_HD inline spm_jst_pair jst_pairs_record(const spm_jst_ref_locus *loci, uint32_t primary1, uint32_t primary2, uint64_t key,
                                            uint32_t b, uint64_t n_pairs, uint64_t n_best, uint64_t n_next)
{
    spm_jst_pair O{};
    const bool proper = key != kJstPairsNoKey;
    if (proper) {
        const uint32_t a = jst_pairs_key_a(key);
        const bool mate1_forward = !jst_pairs_mate2(loci[a].pattern);
        const int32_t t = (int32_t)(loci[b].ref_end - loci[a].ref_begin); // (1 .. 2^31 - 1: concordant)
        O.locus1 = mate1_forward ? a : b;
        O.locus2 = mate1_forward ? b : a;
        O.tlen = mate1_forward ? t : -t;
        O.best = (int32_t)jst_pairs_key_sum(key);
        O.n_pairs = jst_pairs_clamp(n_pairs);
        O.n_best = jst_pairs_clamp(n_best);
        O.n_next = jst_pairs_clamp(n_next);
    } else {
        O.locus1 = primary1;
        O.locus2 = primary2;
        O.best = -1;
    }
    const bool un1 = O.locus1 == kJstPairsNone, un2 = O.locus2 == kJstPairsNone;
    const bool rev1 = !un1 && jst_pairs_reverse(loci[O.locus1].pattern), rev2 = !un2 && jst_pairs_reverse(loci[O.locus2].pattern);
    O.flag1 = jst_pairs_flag(false, proper, un1, un2, rev1, rev2);
    O.flag2 = jst_pairs_flag(true, proper, un2, un1, rev2, rev1);
    return O;
}

struct jst_pairs_totals
{
    uint64_t bad = 0; // records that disagree with the loci + unusable combinations: when not 0 the result means nothing
    uint64_t n_proper = 0, n_unique = 0, n_multi = 0, n_discordant = 0, n_one_mate = 0, n_unmapped = 0, max_window = 0;
};

// The whole rule as a plain loop: out[0 .. n_reads / 2), from the loci and their read summary (strands == 2, n_reads even).
// (The device does the same with one lane per locus and one per pair: jst_pairs.hpp.)
inline jst_pairs_totals jst_pairs_pair_up(const spm_jst_ref_locus *loci, uint64_t n, const spm_jst_read *reads, uint32_t n_reads,
                                          const spm_jst_pair_opts &o, spm_jst_pair *out)
{
    jst_pairs_totals T;
    for (uint32_t p = 0; p < n_reads / 2; ++p) {
        out[p] = spm_jst_pair{};
        const spm_jst_read M[2] = {reads[2 * p], reads[2 * p + 1]};
        if (!jst_pairs_read_ok(loci, n, M[0], 2 * p) || !jst_pairs_read_ok(loci, n, M[1], 2 * p + 1)) {
            T.bad += 1;
            continue;
        }
        uint64_t key = kJstPairsNoKey;
        uint32_t key_partner = kJstPairsNone;
        for (int pass = 0; pass < 2; ++pass) { // the minimum, then the counts against it
            uint64_t c[3] = {0, 0, 0};
            for (int m = 0; m < 2; ++m) {      // the forward loci of mate m against the reverse loci of the other
                const spm_jst_read &F = M[m], &V = M[m ^ 1];
                for (uint32_t a = F.first_locus; a < F.first_locus + F.n_forward; ++a) {
                    const jst_pairs_walked W = jst_pairs_walk(loci, a, V.first_locus + V.n_forward, V.first_locus + V.n_loci, o.min_tlen,
                                                              o.max_tlen, pass ? (long long)jst_pairs_key_sum(key) : -1);
                    if (pass == 0) {
                        T.bad += W.unusable;
                        T.max_window = W.window > T.max_window ? W.window : T.max_window;
                        if (W.partner != kJstPairsNone && jst_pairs_key(W.sum, a) < key) {
                            key = jst_pairs_key(W.sum, a);
                            key_partner = W.partner;
                        }
                    }
                    c[0] += W.n_pairs;
                    c[1] += W.n_best;
                    c[2] += W.n_next;
                }
            }
            if (key == kJstPairsNoKey || pass == 1) {
                out[p] = jst_pairs_record(loci, M[0].primary, M[1].primary, key, key_partner, c[0], c[1], c[2]);
                break;
            }
        }
        const bool proper = (out[p].flag1 & 0x2u) != 0, un1 = (out[p].flag1 & 0x4u) != 0, un2 = (out[p].flag1 & 0x8u) != 0;
        T.n_proper += proper;
        T.n_unique += proper && out[p].n_best == 1;
        T.n_multi += proper && out[p].n_best > 1;
        T.n_discordant += !proper && !un1 && !un2;
        T.n_one_mate += un1 != un2;
        T.n_unmapped += un1 && un2;
    }
    return T;
}

} // namespace spm_hip

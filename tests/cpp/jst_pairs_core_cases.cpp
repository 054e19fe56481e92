// jst_pairs_core_cases.cpp -- the rule of spm_hip_jst_ref_loci_pairs on the host (libspm_amd/csrc/jst_pairs_core.hpp): the
// plain loop over partner windows against an all-combinations brute force written out again here, on random loci lists, and
// hand-worked cases: the bounds of the fragment length, dovetail and containment, ties, the clamp, every flag combination.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <tuple>
#include <vector>

#include "../../libspm_amd/csrc/jst_pairs_core.hpp"
#include "../../libspm_amd/csrc/jst_reads_core.hpp"

using namespace spm_hip;

static int failures = 0, checks = 0;
#define EXPECT_TRUE(cond)                                                                                              \
    do {                                                                                                               \
        ++checks;                                                                                                      \
        if (!(cond)) {                                                                                                 \
            ++failures;                                                                                                \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);                                              \
        }                                                                                                              \
    } while (0)

static spm_jst_ref_locus locus(uint32_t pattern, uint64_t b, uint64_t e, int32_t score)
{
    spm_jst_ref_locus L{};
    L.pattern = pattern;
    L.ref_begin = b;
    L.ref_end = e;
    L.score = score;
    return L;
}

static bool same(const spm_jst_pair &a, const spm_jst_pair &b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// loci in their order, the read summary by the read rule's own plain loop
struct list
{
    std::vector<spm_jst_ref_locus> loci;
    std::vector<spm_jst_read> reads;
    void finish(uint32_t n_reads)
    {
        std::stable_sort(loci.begin(), loci.end(), [](const spm_jst_ref_locus &x, const spm_jst_ref_locus &y) {
            return std::tuple{x.pattern, x.ref_begin} < std::tuple{y.pattern, y.ref_begin};
        });
        reads.assign(n_reads, spm_jst_read{});
        EXPECT_TRUE(jst_reads_summarise(loci.data(), loci.size(), 2, n_reads, reads.data()) == 0);
    }
};

// pair p by all combinations, written out again: nothing of the core but the struct
static spm_jst_pair by_hand(const list &L, uint32_t p, uint32_t min_tlen, uint32_t max_tlen)
{
    std::vector<std::tuple<int64_t, uint32_t, uint32_t>> all; // (sum, a, b)
    for (uint32_t a = 0; a < L.loci.size(); ++a)
        for (uint32_t b = 0; b < L.loci.size(); ++b) {
            const spm_jst_ref_locus &A = L.loci[a], &B = L.loci[b];
            if (A.pattern >> 2 != p || B.pattern >> 2 != p || (A.pattern & 1) || !(B.pattern & 1) || (A.pattern & 2) == (B.pattern & 2))
                continue;
            if (A.ref_begin > B.ref_begin || A.ref_end > B.ref_end)
                continue;
            const uint64_t t = B.ref_end - A.ref_begin;
            if (t >= min_tlen && t <= max_tlen)
                all.push_back({(int64_t)A.score + B.score, a, b});
        }
    spm_jst_pair O{};
    uint32_t l1, l2;
    if (all.empty()) {
        l1 = L.reads[2 * p].primary;
        l2 = L.reads[2 * p + 1].primary;
        O.best = -1;
    } else {
        std::sort(all.begin(), all.end());
        const auto [sum, a, b] = all[0];
        const bool m1f = !(L.loci[a].pattern & 2);
        l1 = m1f ? a : b;
        l2 = m1f ? b : a;
        const int64_t t = (int64_t)(L.loci[b].ref_end - L.loci[a].ref_begin);
        O.tlen = (int32_t)(m1f ? t : -t);
        O.best = (int32_t)sum;
        O.n_pairs = (uint32_t)all.size();
        for (const auto &c : all) {
            O.n_best += std::get<0>(c) == sum;
            O.n_next += std::get<0>(c) == sum + 1;
        }
    }
    O.locus1 = l1;
    O.locus2 = l2;
    const bool un1 = l1 == 0xFFFFFFFFu, un2 = l2 == 0xFFFFFFFFu;
    const bool r1 = !un1 && (L.loci[l1].pattern & 1), r2 = !un2 && (L.loci[l2].pattern & 1);
    const unsigned proper = all.empty() ? 0u : 2u;
    O.flag1 = (uint16_t)(1u | proper | (un1 ? 4u : 0u) | (un2 ? 8u : 0u) | (r1 ? 16u : 0u) | (r2 ? 32u : 0u) | 64u);
    O.flag2 = (uint16_t)(1u | proper | (un2 ? 4u : 0u) | (un1 ? 8u : 0u) | (r2 ? 16u : 0u) | (r1 ? 32u : 0u) | 128u);
    return O;
}

static std::vector<spm_jst_pair> pair_up(const list &L, uint32_t min_tlen, uint32_t max_tlen, jst_pairs_totals *totals = nullptr)
{
    std::vector<spm_jst_pair> out(L.reads.size() / 2);
    const spm_jst_pair_opts o{min_tlen, max_tlen, 0, 0};
    const jst_pairs_totals T = jst_pairs_pair_up(L.loci.data(), L.loci.size(), L.reads.data(), (uint32_t)L.reads.size(), o, out.data());
    EXPECT_TRUE(T.bad == 0);
    if (totals)
        *totals = T;
    return out;
}

static void small_cases()
{
    static_assert(sizeof(spm_jst_pair_opts) == 16 && sizeof(spm_jst_pair) == 32 && sizeof(spm_jst_pairs_stats) == 72, "spm_hip.h");
    // opts
    EXPECT_TRUE(jst_pairs_opts_ok({1, 1, 0, 0}) && jst_pairs_opts_ok({1, 0x7FFFFFFFu, 0, 0}) && jst_pairs_opts_ok({100, 300, 0, 0}));
    EXPECT_TRUE(!jst_pairs_opts_ok({0, 5, 0, 0}) && !jst_pairs_opts_ok({6, 5, 0, 0}) && !jst_pairs_opts_ok({1, 0x80000000u, 0, 0}));
    EXPECT_TRUE(!jst_pairs_opts_ok({1, 5, 1, 0}) && !jst_pairs_opts_ok({1, 5, 0, 1}));
    // keys order as (sum, a)
    const uint32_t sums[] = {0, 1, 7, 0x7FFFFFFFu}, as[] = {0, 1, 64, 0xFFFFFFFEu};
    for (uint32_t s : sums)
        for (uint32_t a : as)
            for (uint32_t s2 : sums)
                for (uint32_t a2 : as) {
                    EXPECT_TRUE((jst_pairs_key(s, a) < jst_pairs_key(s2, a2)) == (s < s2 || (s == s2 && a < a2)));
                    EXPECT_TRUE(jst_pairs_key_sum(jst_pairs_key(s, a)) == s && jst_pairs_key_a(jst_pairs_key(s, a)) == a);
                    EXPECT_TRUE(jst_pairs_key(s, a) != kJstPairsNoKey);
                }
    // sums in 64 bits
    uint32_t s = 9;
    EXPECT_TRUE(jst_pairs_sum(3, 4, s) && s == 7);
    EXPECT_TRUE(jst_pairs_sum(0x7FFFFFFF, 0, s) && s == 0x7FFFFFFFu);
    EXPECT_TRUE(!jst_pairs_sum(0x7FFFFFFF, 1, s) && !jst_pairs_sum(0x40000000, 0x40000000, s) && !jst_pairs_sum(-1, 5, s) && !jst_pairs_sum(5, -1, s));
    EXPECT_TRUE(jst_pairs_clamp(0) == 0 && jst_pairs_clamp(0xFFFFFFFFull) == 0xFFFFFFFFu && jst_pairs_clamp(0x100000000ull) == 0xFFFFFFFFu &&
                jst_pairs_clamp(~0ull) == 0xFFFFFFFFu && jst_pairs_clamp(0xFFFFFFFEull) == 0xFFFFFFFEu);
    // the bounds of the fragment length, min 100, max 300
    const spm_jst_ref_locus a = locus(0, 1000, 1030, 0);
    EXPECT_TRUE(jst_pairs_concordant(a, locus(3, 1070, 1100, 0), 100, 300));   // == min_tlen
    EXPECT_TRUE(!jst_pairs_concordant(a, locus(3, 1069, 1099, 0), 100, 300));  // one below
    EXPECT_TRUE(jst_pairs_concordant(a, locus(3, 1270, 1300, 0), 100, 300));   // == max_tlen
    EXPECT_TRUE(!jst_pairs_concordant(a, locus(3, 1271, 1301, 0), 100, 300));  // one above
    EXPECT_TRUE(!jst_pairs_concordant(a, locus(3, 990, 1120, 0), 100, 300));   // dovetail: b begins left of a
    EXPECT_TRUE(!jst_pairs_concordant(locus(0, 1000, 1200, 0), locus(3, 1050, 1150, 0), 100, 300)); // containment: a ends right of b
    EXPECT_TRUE(jst_pairs_concordant(a, locus(3, 1000, 1100, 0), 100, 300));   // equal begins
    EXPECT_TRUE(jst_pairs_concordant(locus(0, 1000, 1100, 0), locus(3, 1050, 1100, 0), 100, 300)); // equal ends
    EXPECT_TRUE(jst_pairs_concordant(locus(0, 1000, 1000, 0), locus(3, 1100, 1100, 0), 100, 300)); // two anchors inside insertions
    EXPECT_TRUE(jst_pairs_concordant(locus(0, 5, 5, 0), locus(3, 5, 6, 0), 1, 1) && !jst_pairs_concordant(locus(0, 5, 5, 0), locus(3, 5, 5, 0), 1, 1));
    EXPECT_TRUE(jst_pairs_concordant(locus(0, ~0ull - 10, ~0ull - 5, 0), locus(3, ~0ull - 8, ~0ull, 0), 1, 0x7FFFFFFFu)); // no wrap
    // every flag combination
    for (int m = 0; m < 64; ++m) {
        const bool mate2 = m & 1, proper = m & 2, su = m & 4, ou = m & 8, sr = m & 16, orv = m & 32;
        const uint16_t f = jst_pairs_flag(mate2, proper, su, ou, sr, orv);
        EXPECT_TRUE((f & 1) && !!(f & 2) == proper && !!(f & 4) == su && !!(f & 8) == ou && !!(f & 16) == sr && !!(f & 32) == orv);
        EXPECT_TRUE(!!(f & 64) == !mate2 && !!(f & 128) == mate2 && (f & ~0xFFu) == 0);
    }
}

static void worked_cases()
{
    {   // the pair of the primaries is not the primary pair (case 1 of spm_hip.h); pair 1: mate 1 reverse (case 2)
        list L;
        L.loci = {locus(0, 1000, 1030, 0), locus(3, 1170, 1200, 1), locus(3, 7000, 7030, 0), locus(6, 500, 530, 0), locus(5, 720, 750, 0)};
        L.finish(4);
        EXPECT_TRUE(L.reads[1].primary == 2);
        jst_pairs_totals T;
        const auto out = pair_up(L, 100, 300, &T);
        EXPECT_TRUE(out[0].locus1 == 0 && out[0].locus2 == 1 && out[0].tlen == 200 && out[0].best == 1 && out[0].n_pairs == 1 &&
                    out[0].n_best == 1 && out[0].n_next == 0 && out[0].flag1 == 0x63 && out[0].flag2 == 0x93);
        EXPECT_TRUE(out[1].locus1 == 3 && out[1].locus2 == 4 && out[1].tlen == -250 && out[1].best == 0 && out[1].flag1 == 0x53 &&
                    out[1].flag2 == 0xA3);
        EXPECT_TRUE(T.n_proper == 2 && T.n_unique == 2 && T.n_multi == 0 && T.n_discordant + T.n_one_mate + T.n_unmapped == 0);
        EXPECT_TRUE(T.max_window == 1); // (7000 lies outside every window)
        for (uint32_t p = 0; p < 2; ++p)
            EXPECT_TRUE(same(out[p], by_hand(L, p, 100, 300)));
    }
    {   // bounds: pairs 0..3 have fragment 100, 99, 300, 301; 4 a dovetail; 5 a containment; 6 same strand; 7 one mate (mate 2);
        // 8 one mate (mate 1); 9 unmapped
        list L;
        const uint64_t bb[] = {1070, 1069, 1270, 1271};
        for (uint32_t p = 0; p < 4; ++p) {
            L.loci.push_back(locus(4 * p, 1000, 1030, 0));
            L.loci.push_back(locus(4 * p + 3, bb[p], bb[p] + 30, 0));
        }
        L.loci.push_back(locus(16, 1000, 1030, 0));
        L.loci.push_back(locus(19, 990, 1120, 0));
        L.loci.push_back(locus(20, 1000, 1200, 0));
        L.loci.push_back(locus(23, 1050, 1150, 0));
        L.loci.push_back(locus(24, 1000, 1030, 0));
        L.loci.push_back(locus(26, 1170, 1200, 1));
        L.loci.push_back(locus(25 + 4, 1000, 1030, 2)); // pair 7: only mate 1, reverse
        L.loci.push_back(locus(32 + 2, 1000, 1030, 0)); // pair 8: only mate 2, forward
        L.finish(20);
        jst_pairs_totals T;
        const auto out = pair_up(L, 100, 300, &T);
        const int32_t tl[] = {100, 0, 300, 0};
        for (uint32_t p = 0; p < 4; ++p) {
            EXPECT_TRUE(out[p].tlen == tl[p] && (out[p].best == 0) == (tl[p] != 0) && out[p].locus1 == 2 * p && out[p].locus2 == 2 * p + 1);
            EXPECT_TRUE(out[p].flag1 == (tl[p] ? 0x63 : 0x61) && out[p].flag2 == (tl[p] ? 0x93 : 0x91));
        }
        EXPECT_TRUE(out[4].best == -1 && out[4].flag1 == 0x61 && out[5].best == -1 && out[5].n_pairs == 0);
        EXPECT_TRUE(out[6].best == -1 && out[6].flag1 == 0x41 && out[6].flag2 == 0x81 && out[6].locus1 == 12 && out[6].locus2 == 13);
        EXPECT_TRUE(out[7].locus1 == 14 && out[7].locus2 == 0xFFFFFFFFu && out[7].flag1 == (0x1 | 0x8 | 0x10 | 0x40) &&
                    out[7].flag2 == (0x1 | 0x4 | 0x20 | 0x80) && out[7].tlen == 0);
        EXPECT_TRUE(out[8].locus1 == 0xFFFFFFFFu && out[8].locus2 == 15 && out[8].flag1 == (0x1 | 0x4 | 0x40) && out[8].flag2 == (0x1 | 0x8 | 0x80));
        EXPECT_TRUE(out[9].locus1 == 0xFFFFFFFFu && out[9].locus2 == 0xFFFFFFFFu && out[9].flag1 == 0x4D && out[9].flag2 == 0x8D &&
                    out[9].best == -1 && out[9].tlen == 0 && out[9].n_pairs == 0 && out[9].n_best == 0 && out[9].n_next == 0);
        EXPECT_TRUE(T.n_proper == 2 && T.n_discordant == 5 && T.n_one_mate == 2 && T.n_unmapped == 1 && T.n_unique == 2);
        for (uint32_t p = 0; p < 10; ++p)
            EXPECT_TRUE(same(out[p], by_hand(L, p, 100, 300)));
    }
    {   // a tie: two forward loci of mate 1, two reverse loci of mate 2, all four combinations concordant; sums 1, 1, 2, 2 --
        // the smallest a, then the smallest b of the best partner score; n_best 2, n_next 2
        list L;
        L.loci = {locus(0, 1000, 1030, 0), locus(0, 1010, 1040, 1), locus(3, 1150, 1180, 1), locus(3, 1160, 1190, 1)};
        L.finish(2);
        auto out = pair_up(L, 100, 300);
        EXPECT_TRUE(out[0].locus1 == 0 && out[0].locus2 == 2 && out[0].best == 1 && out[0].n_pairs == 4 && out[0].n_best == 2 &&
                    out[0].n_next == 2 && out[0].tlen == 180);
        EXPECT_TRUE(same(out[0], by_hand(L, 0, 100, 300)));
        // the sum decides before the indices: the best combination is the larger a with the larger b
        L.loci = {locus(0, 1000, 1030, 1), locus(0, 1010, 1040, 0), locus(3, 1150, 1180, 1), locus(3, 1160, 1190, 0)};
        L.finish(2);
        out = pair_up(L, 100, 300);
        EXPECT_TRUE(out[0].best == 0 && out[0].locus1 == 1 && out[0].locus2 == 3 && out[0].n_best == 1 && out[0].n_next == 2 && out[0].n_pairs == 4);
        L.loci = {locus(0, 1000, 1030, 0), locus(0, 1010, 1040, 0), locus(3, 1150, 1180, 0), locus(3, 1160, 1190, 0)};
        L.finish(2);
        out = pair_up(L, 100, 300);
        EXPECT_TRUE(out[0].best == 0 && out[0].locus1 == 0 && out[0].locus2 == 2 && out[0].n_best == 4 && out[0].n_next == 0);
        // both directions in one pair: mate 2 forward with mate 1 reverse is better
        L.loci = {locus(0, 1000, 1030, 1), locus(1, 3200, 3230, 0), locus(2, 3000, 3030, 0), locus(3, 1150, 1180, 1)};
        L.finish(2);
        out = pair_up(L, 100, 300);
        EXPECT_TRUE(out[0].best == 0 && out[0].locus1 == 1 && out[0].locus2 == 2 && out[0].tlen == -230 && out[0].n_pairs == 2 &&
                    out[0].n_best == 1 && out[0].n_next == 0 && out[0].flag1 == 0x53);
        EXPECT_TRUE(same(out[0], by_hand(L, 0, 100, 300)));
    }
    {   // the clamp: the record holds 0xFFFFFFFF for anything above
        list L;
        L.loci = {locus(0, 1000, 1030, 0), locus(3, 1150, 1180, 0)};
        L.finish(2);
        const spm_jst_pair O = jst_pairs_record(L.loci.data(), 0, 1, jst_pairs_key(0, 0), 1, 0x100000000ull, 0xFFFFFFFFull, 0x1FFFFFFFFull);
        EXPECT_TRUE(O.n_pairs == 0xFFFFFFFFu && O.n_best == 0xFFFFFFFFu && O.n_next == 0xFFFFFFFFu && O.tlen == 180);
        const spm_jst_pair Q = jst_pairs_record(L.loci.data(), 0, 1, jst_pairs_key(0, 0), 1, 0xFFFFFFFEull, 5, 0);
        EXPECT_TRUE(Q.n_pairs == 0xFFFFFFFEu && Q.n_best == 5 && Q.n_next == 0);
    }
    {   // a sum that does not fit is counted, as is a summary that disagrees with the loci; the longest tlen
        list L;
        L.loci = {locus(0, 1000, 1030, 0x7FFFFFFF), locus(3, 1150, 1180, 1)};
        L.finish(2);
        std::vector<spm_jst_pair> out(1);
        const spm_jst_pair_opts o{100, 300, 0, 0};
        EXPECT_TRUE(jst_pairs_pair_up(L.loci.data(), 2, L.reads.data(), 2, o, out.data()).bad == 1);
        L.loci[0].score = 0x7FFFFFFE;
        EXPECT_TRUE(jst_pairs_pair_up(L.loci.data(), 2, L.reads.data(), 2, o, out.data()).bad == 0 && out[0].best == 0x7FFFFFFF && out[0].n_next == 0);
        list M = L;
        M.reads[1].first_locus = 2;   // the run leaves the loci
        EXPECT_TRUE(jst_pairs_pair_up(M.loci.data(), 2, M.reads.data(), 2, o, out.data()).bad == 1);
        M = L;
        M.reads[1].n_forward = 1;     // the reverse locus called forward: the tail names another strand
        EXPECT_TRUE(jst_pairs_pair_up(M.loci.data(), 2, M.reads.data(), 2, o, out.data()).bad == 1);
        M = L;
        M.reads[0].primary = 1;       // the primary outside the run
        EXPECT_TRUE(jst_pairs_pair_up(M.loci.data(), 2, M.reads.data(), 2, o, out.data()).bad == 1);
        M = L;
        M.reads[0] = jst_reads_unmapped(0); // a read that has loci called unmapped: its partner's record still holds
        M.reads[1].first_locus = 0;
        M.reads[1].n_loci = 2;              // ... but this run's head names read 0
        EXPECT_TRUE(jst_pairs_pair_up(M.loci.data(), 2, M.reads.data(), 2, o, out.data()).bad == 1);
        EXPECT_TRUE(jst_pairs_covers(L.reads[0], 2, 0, 0) && !jst_pairs_covers(L.reads[0], 2, 1, 0) && !jst_pairs_covers(L.reads[0], 2, 0, 1) &&
                    jst_pairs_covers(L.reads[1], 2, 1, 3) && !jst_pairs_covers(L.reads[1], 2, 1, 2) && !jst_pairs_covers(L.reads[1], 1, 1, 3));
        list W;
        W.loci = {locus(0, 0, 30, 0), locus(3, 0x7FFFFFFFull - 30, 0x7FFFFFFFull, 0), locus(3, 0x7FFFFFFFull - 29, 0x80000000ull, 0)};
        W.finish(2);
        const auto big = pair_up(W, 1, 0x7FFFFFFFu);
        EXPECT_TRUE(big[0].tlen == 0x7FFFFFFF && big[0].n_pairs == 1 && big[0].locus2 == 1);
    }
    {   // no loci, no reads
        list L;
        L.finish(6);
        jst_pairs_totals T;
        const auto out = pair_up(L, 1, 10, &T);
        for (const spm_jst_pair &O : out)
            EXPECT_TRUE(O.flag1 == 0x4D && O.flag2 == 0x8D && O.locus1 == 0xFFFFFFFFu && O.locus2 == 0xFFFFFFFFu && O.best == -1);
        EXPECT_TRUE(T.n_unmapped == 3 && T.max_window == 0);
        const spm_jst_pair_opts o{1, 10, 0, 0};
        EXPECT_TRUE(jst_pairs_pair_up(nullptr, 0, nullptr, 0, o, nullptr).bad == 0);
    }
}

static void random_cases()
{
    uint64_t z = 20261019;
    auto rnd = [&](uint32_t m) {
        z = z * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)(z >> 33) % m;
    };
    uint64_t proper = 0, multi = 0, windows = 0, fallbacks = 0, differs = 0;
    for (int trial = 0; trial < 120; ++trial) {
        const uint32_t n_pairs = rnd(41), span = 200 + rnd(1500);
        list L;
        for (uint32_t p = 0; p < 4 * n_pairs; ++p)
            for (uint32_t c = rnd(3) ? rnd(13) : 0; c > 0; --c) {
                const uint64_t b = rnd(span), len = rnd(8) ? 20 + rnd(20) : 0; // (some anchors inside insertions)
                L.loci.push_back(locus(p, b, b + len, (int32_t)rnd(4)));
            }
        L.finish(2 * n_pairs);
        const uint32_t min_tlen = 1 + rnd(120), max_tlen = min_tlen + rnd(400);
        jst_pairs_totals T;
        const auto out = pair_up(L, min_tlen, max_tlen, &T);
        uint64_t n_proper = 0;
        for (uint32_t p = 0; p < n_pairs; ++p) {
            const spm_jst_pair want = by_hand(L, p, min_tlen, max_tlen);
            EXPECT_TRUE(same(out[p], want));
            n_proper += want.best >= 0;
            multi += want.n_best > 1;
            fallbacks += want.best < 0 && want.locus1 != 0xFFFFFFFFu && want.locus2 != 0xFFFFFFFFu;
            differs += want.best >= 0 && (want.locus1 != L.reads[2 * p].primary || want.locus2 != L.reads[2 * p + 1].primary);
        }
        EXPECT_TRUE(T.n_proper == n_proper);
        EXPECT_TRUE(T.n_proper + T.n_discordant + T.n_one_mate + T.n_unmapped == n_pairs && T.n_unique + T.n_multi == T.n_proper);
        proper += n_proper;
        windows += T.max_window >= 3;
    }
    EXPECT_TRUE(proper > 500 && multi > 100 && windows > 60 && fallbacks > 50 && differs > 100);
}

int main()
{
    small_cases();
    worked_cases();
    random_cases();
    std::printf("%d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}

// jst_reads_core_cases.cpp -- the rule of spm_hip_jst_ref_loci_reads on the host (libspm_amd/csrc/jst_reads_core.hpp): key
// packing, classification, and the plain loop over loci against a summary written out again here.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

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

static spm_jst_ref_locus locus(uint32_t pattern, int32_t score, int32_t ref_score)
{
    spm_jst_ref_locus L{};
    L.pattern = pattern;
    L.score = score;
    L.ref_score = ref_score;
    return L;
}

static bool same(const spm_jst_read &a, const spm_jst_read &b) { return std::memcmp(&a, &b, sizeof a) == 0; }

static void key_cases()
{
    static_assert(sizeof(spm_jst_read) == 32, "spm_hip.h states 32 bytes");
    static_assert(sizeof(spm_jst_reads_stats) == 48, "spm_hip.h states 48 bytes");
    const int32_t scores[] = {0, 1, 2, 255, 65536, 0x7FFFFFFE, 0x7FFFFFFF};
    const uint32_t loci[] = {0, 1, 63, 64, 0x7FFFFFFF, 0xFFFFFFFE, 0xFFFFFFFF};
    for (int32_t s : scores)
        for (uint32_t l : loci) {
            const uint64_t k = jst_reads_key(s, l);
            EXPECT_TRUE(jst_reads_key_score(k) == s && jst_reads_key_locus(k) == l);
            EXPECT_TRUE(k != kJstReadsNoKey || (s < 0));
            for (int32_t s2 : scores)
                for (uint32_t l2 : loci) // the order of the keys is the order of (score, locus)
                    EXPECT_TRUE((k < jst_reads_key(s2, l2)) == (s < s2 || (s == s2 && l < l2)));
        }
    EXPECT_TRUE(jst_reads_key(-1, 0xFFFFFFFFu) == kJstReadsNoKey); // why a negative score is unusable
    // classification; best + 1 at INT32_MAX does not wrap
    EXPECT_TRUE(jst_reads_class(3, 3) == 0 && jst_reads_class(4, 3) == 1 && jst_reads_class(5, 3) == 2 && jst_reads_class(2, 3) == 2);
    EXPECT_TRUE(jst_reads_class(0x7FFFFFFF, 0x7FFFFFFF) == 0);
    EXPECT_TRUE(jst_reads_class((int32_t)0x80000000u, 0x7FFFFFFF) == 2); // INT32_MIN is not best + 1
    EXPECT_TRUE(jst_reads_class(0x7FFFFFFF, 0x7FFFFFFE) == 1);
    EXPECT_TRUE(jst_reads_class(0, -1) == 1);
    // reads and strands
    EXPECT_TRUE(jst_reads_read(7, 1) == 7 && jst_reads_read(7, 2) == 3 && jst_reads_read(6, 2) == 3);
    EXPECT_TRUE(jst_reads_forward(7, 1) && !jst_reads_forward(7, 2) && jst_reads_forward(6, 2));
    EXPECT_TRUE(jst_reads_usable(5, 0, 2, 3) && !jst_reads_usable(6, 0, 2, 3) && !jst_reads_usable(5, -1, 2, 3));
    EXPECT_TRUE(jst_reads_usable(2, 0, 1, 3) && !jst_reads_usable(3, 0, 1, 3) && !jst_reads_usable(0, 0, 1, 0));
    EXPECT_TRUE(jst_reads_usable(0xFFFFFFFEu, 0, 1, 0xFFFFFFFFu) && !jst_reads_usable(0xFFFFFFFFu, 0, 1, 0xFFFFFFFFu));
    EXPECT_TRUE(jst_reads_usable(0xFFFFFFFDu, 0, 2, 0x7FFFFFFFu) && !jst_reads_usable(0xFFFFFFFEu, 0, 2, 0x7FFFFFFFu));
}

// the summary of one read, written out again: sort its loci by (score, index)
static spm_jst_read by_hand(const std::vector<spm_jst_ref_locus> &L, uint32_t strands, uint32_t r)
{
    std::vector<std::pair<int64_t, uint32_t>> mine;
    uint32_t first = 0, fwd = 0;
    for (uint32_t i = 0; i < L.size(); ++i) {
        if (L[i].pattern / strands < r)
            first = i + 1;
        if (L[i].pattern / strands == r) {
            mine.push_back({L[i].score, i});
            fwd += L[i].pattern % strands == 0;
        }
    }
    spm_jst_read R{};
    R.first_locus = first;
    R.primary = 0xFFFFFFFFu;
    R.best = R.best_ref_score = -1;
    if (mine.empty())
        return R;
    std::sort(mine.begin(), mine.end());
    R.n_loci = (uint32_t)mine.size();
    R.n_forward = fwd;
    R.primary = mine[0].second;
    R.best = (int32_t)mine[0].first;
    R.best_ref_score = L[R.primary].ref_score;
    for (const auto &m : mine) {
        R.n_best += m.first == mine[0].first;
        R.n_next += m.first == mine[0].first + 1;
    }
    return R;
}

static void summary_cases()
{
    // stranded, 5 reads: read 0 unmapped (index 0), read 1 ties between strands (forward wins by index), read 2 unmapped
    // between two mapped ones, read 3 reverse only with best + 1, read 4 unmapped at the end
    std::vector<spm_jst_ref_locus> L = {locus(2, 1, 4), locus(2, 0, 9), locus(2, 0, 3), locus(3, 0, 5), locus(3, 1, 6),
                                        locus(7, 2, 2), locus(7, 1, 8), locus(7, 2, 1)};
    std::vector<spm_jst_read> out(5);
    EXPECT_TRUE(jst_reads_summarise(L.data(), L.size(), 2, 5, out.data()) == 0);
    for (uint32_t r = 0; r < 5; ++r)
        EXPECT_TRUE(same(out[r], by_hand(L, 2, r)));
    EXPECT_TRUE(out[0].n_loci == 0 && out[0].first_locus == 0 && out[0].primary == 0xFFFFFFFFu && out[0].best == -1);
    EXPECT_TRUE(out[1].first_locus == 0 && out[1].n_loci == 5 && out[1].n_forward == 3 && out[1].primary == 1 && out[1].best == 0 &&
                out[1].best_ref_score == 9 && out[1].n_best == 3 && out[1].n_next == 2);
    EXPECT_TRUE(out[2].n_loci == 0 && out[2].first_locus == 5 && out[2].best_ref_score == -1);
    EXPECT_TRUE(out[3].first_locus == 5 && out[3].n_loci == 3 && out[3].n_forward == 0 && out[3].primary == 6 && out[3].n_best == 1 &&
                out[3].n_next == 2);
    EXPECT_TRUE(out[4].n_loci == 0 && out[4].first_locus == 8);
    // the same loci as a plain set of 8 reads
    out.assign(8, spm_jst_read{});
    EXPECT_TRUE(jst_reads_summarise(L.data(), L.size(), 1, 8, out.data()) == 0);
    for (uint32_t r = 0; r < 8; ++r) {
        EXPECT_TRUE(same(out[r], by_hand(L, 1, r)));
        EXPECT_TRUE(out[r].n_forward == out[r].n_loci);
    }
    // a pattern out of range, a negative score: counted, nothing else
    EXPECT_TRUE(jst_reads_summarise(L.data(), L.size(), 2, 3, out.data()) == 3);
    EXPECT_TRUE(jst_reads_summarise(L.data(), L.size(), 1, 7, out.data()) == 3);
    L[4].score = -1;
    EXPECT_TRUE(jst_reads_summarise(L.data(), L.size(), 2, 5, out.data()) == 1);
    // no loci, no reads
    out.assign(3, spm_jst_read{});
    EXPECT_TRUE(jst_reads_summarise(nullptr, 0, 2, 3, out.data()) == 0);
    for (uint32_t r = 0; r < 3; ++r)
        EXPECT_TRUE(same(out[r], jst_reads_unmapped(0)));
    EXPECT_TRUE(jst_reads_summarise(L.data(), 0, 2, 0, nullptr) == 0);
    // best at INT32_MAX: nothing is "next"
    std::vector<spm_jst_ref_locus> M = {locus(0, 0x7FFFFFFF, 1), locus(1, 0x7FFFFFFF, 2)};
    out.assign(1, spm_jst_read{});
    EXPECT_TRUE(jst_reads_summarise(M.data(), M.size(), 2, 1, out.data()) == 0);
    EXPECT_TRUE(out[0].best == 0x7FFFFFFF && out[0].n_best == 2 && out[0].n_next == 0 && out[0].primary == 0 && out[0].n_forward == 1);
    // random loci lists against the hand-written summary
    uint64_t z = 99;
    auto rnd = [&](uint32_t m) {
        z = z * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)(z >> 33) % m;
    };
    for (int trial = 0; trial < 300; ++trial) {
        const uint32_t strands = 1 + rnd(2), n_reads = 1 + rnd(12);
        std::vector<spm_jst_ref_locus> R;
        for (uint32_t p = 0; p < strands * n_reads; ++p)
            for (uint32_t c = rnd(4) ? rnd(5) : 0; c > 0; --c)
                R.push_back(locus(p, (int32_t)rnd(3), (int32_t)rnd(9)));
        out.assign(n_reads, spm_jst_read{});
        EXPECT_TRUE(jst_reads_summarise(R.data(), R.size(), strands, n_reads, out.data()) == 0);
        for (uint32_t r = 0; r < n_reads; ++r)
            EXPECT_TRUE(same(out[r], by_hand(R, strands, r)));
    }
}

int main()
{
    key_cases();
    summary_cases();
    std::printf("%d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}

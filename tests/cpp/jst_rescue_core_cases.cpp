// jst_rescue_core_cases.cpp -- the rule of spm_hip_jst_pairs_rescue on the host (libspm_amd/csrc/jst_rescue_core.hpp): the jobs
// of a pair record, the window and its clipping at 0 and at N, the geometry of the 64 chunks, key packing, the record and its
// classification on the worked cases of spm_hip.h, and the exactness claim of the search: a plain dynamic-programming
// search over the whole window, written out again here, equals the bit-vector search cut into 64 cold-started chunks.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../libspm_amd/csrc/jst_rescue_core.hpp"

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

static spm_jst_ref_locus locus(uint32_t pattern, uint64_t b, uint64_t e)
{
    spm_jst_ref_locus L{};
    L.pattern = pattern;
    L.ref_begin = b;
    L.ref_end = e;
    return L;
}

static spm_jst_pair pair_record(uint32_t l1, uint32_t l2, bool proper, bool rev1, bool rev2)
{
    spm_jst_pair R{};
    R.locus1 = l1;
    R.locus2 = l2;
    const bool un1 = l1 == kJstPairsNone, un2 = l2 == kJstPairsNone;
    R.flag1 = jst_pairs_flag(false, proper, un1, un2, rev1, rev2);
    R.flag2 = jst_pairs_flag(true, proper, un2, un1, rev2, rev1);
    return R;
}

static spm_jst_read read_record(uint32_t primary)
{
    spm_jst_read M{};
    M.primary = primary;
    return M;
}

static void jobs_cases()
{
    const uint32_t X = kJstPairsNone;
    EXPECT_TRUE(jst_rescue_anchors(pair_record(3, 4, true, false, true)) == 0);
    EXPECT_TRUE(jst_rescue_anchors(pair_record(X, X, false, false, false)) == 0);
    EXPECT_TRUE(jst_rescue_anchors(pair_record(3, X, false, false, false)) == 1);
    EXPECT_TRUE(jst_rescue_anchors(pair_record(X, 4, false, false, true)) == 2);
    EXPECT_TRUE(jst_rescue_anchors(pair_record(3, 4, false, false, false)) == 3);
    EXPECT_TRUE(jst_rescue_job_count(0) == 0 && jst_rescue_job_count(1) == 1 && jst_rescue_job_count(2) == 1 && jst_rescue_job_count(3) == 2);
    // q = 4 p + 2 (mate of Y) + (1 - strand bit of A): anchor mate 1 forward (pattern 4p) -> mate 2 reverse (4p + 3), ...
    EXPECT_TRUE(jst_rescue_needle(5, 0, 20) == 23);
    EXPECT_TRUE(jst_rescue_needle(5, 0, 21) == 22);
    EXPECT_TRUE(jst_rescue_needle(5, 1, 22) == 21);
    EXPECT_TRUE(jst_rescue_needle(5, 1, 23) == 20);
    EXPECT_TRUE(jst_rescue_needle(0, 1, 3) == 0);
    // the agreement of a pair record with the read summary, the loci and the reference (pair 1: patterns 4 .. 7)
    const spm_jst_ref_locus loci[3] = {locus(4, 100, 130), locus(7, 300, 330), locus(6, 900, 1001)};
    const uint64_t N = 1000;
    EXPECT_TRUE(jst_rescue_pair_ok(loci, 3, read_record(0), read_record(1), pair_record(0, 1, false, false, true), 1, N));
    EXPECT_TRUE(jst_rescue_pair_ok(loci, 3, read_record(0), read_record(X), pair_record(0, X, false, false, false), 1, N));
    EXPECT_TRUE(jst_rescue_pair_ok(loci, 3, read_record(X), read_record(X), pair_record(X, X, false, false, false), 1, N));
    EXPECT_TRUE(jst_rescue_pair_ok(loci, 3, read_record(2), read_record(2), pair_record(0, 1, true, false, true), 1, N)); // proper: any locus of the read
    EXPECT_TRUE(!jst_rescue_pair_ok(loci, 3, read_record(0), read_record(1), pair_record(3, 1, false, false, true), 1, N));  // beyond the loci
    EXPECT_TRUE(!jst_rescue_pair_ok(loci, 3, read_record(0), read_record(1), pair_record(0, 0xFFFFFFF0u, false, false, true), 1, N));
    EXPECT_TRUE(!jst_rescue_pair_ok(loci, 3, read_record(0), read_record(1), pair_record(0, 1, false, false, true), 2, N));  // another pair
    EXPECT_TRUE(!jst_rescue_pair_ok(loci, 3, read_record(1), read_record(0), pair_record(1, 0, false, true, false), 1, N));  // the mates swapped
    EXPECT_TRUE(!jst_rescue_pair_ok(loci, 3, read_record(0), read_record(1), pair_record(0, 1, false, true, true), 1, N));   // the strand
    EXPECT_TRUE(!jst_rescue_pair_ok(loci, 3, read_record(0), read_record(2), pair_record(0, 2, false, false, false), 1, N)); // ref_end > N
    EXPECT_TRUE(jst_rescue_pair_ok(loci, 3, read_record(0), read_record(2), pair_record(0, 2, false, false, false), 1, 1001));
    EXPECT_TRUE(!jst_rescue_pair_ok(loci, 3, read_record(2), read_record(1), pair_record(0, 1, false, false, true), 1, N));  // not the primary
    spm_jst_pair odd = pair_record(0, X, false, false, false);
    odd.flag1 &= (uint16_t)~0x8u; // mate 2 has no locus, the flag says it has
    EXPECT_TRUE(!jst_rescue_pair_ok(loci, 3, read_record(0), read_record(X), odd, 1, N));
    const spm_jst_ref_locus turned[1] = {locus(4, 130, 100)};
    EXPECT_TRUE(!jst_rescue_pair_ok(turned, 1, read_record(0), read_record(X), pair_record(0, X, false, false, false), 1, N));
    spm_jst_rescue_opts o{100, 300, 6, 0, 0};
    EXPECT_TRUE(jst_rescue_opts_ok(o));
    o.min_tlen = 0;
    EXPECT_TRUE(!jst_rescue_opts_ok(o));
    o = {301, 300, 6, 0, 0};
    EXPECT_TRUE(!jst_rescue_opts_ok(o));
    o = {1, 0x80000000u, 6, 0, 0};
    EXPECT_TRUE(!jst_rescue_opts_ok(o));
    o = {1, 0x7FFFFFFFu, 0xFFFFFFFFu, 0, 0};
    EXPECT_TRUE(jst_rescue_opts_ok(o));
    o.flags = 1;
    EXPECT_TRUE(!jst_rescue_opts_ok(o));
}

static void window_cases()
{
    // the worked cases of spm_hip.h: min_tlen 100, max_tlen 300, N = 10000
    jst_rescue_window W = jst_rescue_window_of(1000, 1030, false, 100, 300, 10000);
    EXPECT_TRUE(W.lo == 1000 && W.hi == 1300 && W.e_first == 1100 && W.n_ends == 201);
    W = jst_rescue_window_of(720, 750, true, 100, 300, 10000);
    EXPECT_TRUE(W.lo == 450 && W.hi == 750 && W.e_first == 451 && W.n_ends == 300);
    W = jst_rescue_window_of(9800, 9830, false, 100, 300, 10000);
    EXPECT_TRUE(W.lo == 9800 && W.hi == 10000 && W.e_first == 9900 && W.n_ends == 101);
    W = jst_rescue_window_of(9950, 9980, false, 100, 300, 10000);
    EXPECT_TRUE(W.lo == 9950 && W.hi == 10000 && W.n_ends == 0);
    W = jst_rescue_window_of(9900, 9930, false, 100, 300, 10000); // exactly one end, N itself
    EXPECT_TRUE(W.e_first == 10000 && W.n_ends == 1);
    W = jst_rescue_window_of(170, 200, true, 100, 300, 10000);
    EXPECT_TRUE(W.lo == 0 && W.hi == 200 && W.e_first == 1 && W.n_ends == 200);
    W = jst_rescue_window_of(0, 0, true, 100, 300, 10000);
    EXPECT_TRUE(W.n_ends == 0);
    W = jst_rescue_window_of(270, 300, true, 100, 300, 10000);
    EXPECT_TRUE(W.lo == 0 && W.n_ends == 300);
    W = jst_rescue_window_of(271, 301, true, 100, 300, 10000);
    EXPECT_TRUE(W.lo == 1 && W.e_first == 2 && W.n_ends == 300);
    // an anchor longer than min_tlen: the first end is its own
    W = jst_rescue_window_of(1000, 1150, false, 100, 300, 10000);
    EXPECT_TRUE(W.e_first == 1150 && W.n_ends == 151);
    // ... and longer than max_tlen: nothing
    W = jst_rescue_window_of(1000, 1400, false, 100, 300, 10000);
    EXPECT_TRUE(W.n_ends == 0);
    // the largest bounds at the far end of 64 bits do not wrap
    W = jst_rescue_window_of(~0ull - 10, ~0ull - 5, false, 1, 0x7FFFFFFFu, ~0ull - 1);
    EXPECT_TRUE(W.hi == ~0ull - 1 && W.e_first == ~0ull - 5 && W.n_ends == 5);
    W = jst_rescue_window_of(5, 10, true, 1, 0x7FFFFFFFu, ~0ull);
    EXPECT_TRUE(W.lo == 0 && W.n_ends == 10);
}

static void chunk_cases()
{
    for (uint32_t n_ends : {0u, 1u, 63u, 64u, 65u, 1000u})
        for (uint64_t lo : {0ull, 7ull, 5000ull})
            for (uint32_t m : {1u, 33u, 256u})
                for (uint32_t k : {0u, 6u}) {
                    jst_rescue_window W;
                    W.lo = lo;
                    W.e_first = lo + 1 + (n_ends % 7) * 20;
                    W.n_ends = n_ends;
                    W.hi = W.e_first + n_ends;
                    uint64_t next = W.e_first, total = 0;
                    uint32_t longest = 0, shortest = ~0u;
                    bool ok = true;
                    for (uint32_t i = 0; i < kJstRescueLanes; ++i) {
                        const jst_rescue_chunk C = jst_rescue_chunk_of(W, i, m, k);
                        ok = ok && C.first == next && C.start >= lo && C.start < C.first;
                        ok = ok && (C.start == lo || C.start == C.first - 1 - (m + k));
                        ok = ok && (C.start == lo ? C.first - lo <= 1ull + m + k : true);
                        next += C.len;
                        total += C.len;
                        longest = std::max(longest, C.len);
                        shortest = std::min(shortest, C.len);
                        if (i > 0)
                            ok = ok && C.len <= jst_rescue_chunk_of(W, i - 1, m, k).len; // the longer chunks come first
                    }
                    EXPECT_TRUE(ok);
                    EXPECT_TRUE(total == n_ends && next == W.e_first + n_ends);
                    EXPECT_TRUE(longest - shortest <= 1 && longest == (n_ends + 63) / 64);
                }
    EXPECT_TRUE(jst_rescue_key_d(jst_rescue_key(6, 123)) == 6 && jst_rescue_key_rel(jst_rescue_key(6, 123)) == 123);
    EXPECT_TRUE(jst_rescue_key(2, 500) < jst_rescue_key(3, 1));
    EXPECT_TRUE(jst_rescue_key(2, 499) < jst_rescue_key(2, 500));
    EXPECT_TRUE(jst_rescue_key(256, 0x7FFFFFFFu) < kJstRescueNoKey);
    EXPECT_TRUE(jst_rescue_key_rel(jst_rescue_key(0, 0x7FFFFFFFu)) == 0x7FFFFFFFu);
}

static void record_cases()
{
    // case 1 of spm_hip.h: mate 1 forward at [1000,1030) (pair 2: pattern 8), candidate [1170,1200) with 4 edits
    spm_jst_rescue O = jst_rescue_record(locus(8, 1000, 1030), 17, 2, 0, 11, true, 1170, 1200, 4, 9, 5, 100, 300);
    EXPECT_TRUE(O.status == SPM_RESCUE_RESCUED && O.tlen == 200 && O.flag == 0x93 && O.score == 4 && O.ref_begin == 1170 && O.ref_end == 1200);
    EXPECT_TRUE(O.pair == 2 && O.pattern == 11 && O.anchor == 17 && O.cigar_off == 9 && O.cigar_len == 5);
    // the same with mate 2 as the forward anchor: mate 1 is the reverse one, tlen of mate 1 is negative
    O = jst_rescue_record(locus(10, 1000, 1030), 17, 2, 1, 9, true, 1170, 1200, 4, 0, 1, 100, 300);
    EXPECT_TRUE(O.status == SPM_RESCUE_RESCUED && O.tlen == -200 && O.flag == 0x53);
    // case 2: mate 2 reverse at [720,750) (pattern 11), mate 1 forward rescued
    O = jst_rescue_record(locus(11, 720, 750), 3, 2, 1, 8, true, 500, 530, 3, 0, 3, 100, 300);
    EXPECT_TRUE(O.status == SPM_RESCUE_RESCUED && O.tlen == 250 && O.flag == 0x63);
    O = jst_rescue_record(locus(11, 720, 750), 3, 2, 1, 8, true, 700, 730, 3, 0, 3, 100, 300); // 50 < min_tlen
    EXPECT_TRUE(O.status == SPM_RESCUE_NOT_CONCORDANT && O.tlen == 0 && O.flag == 0x61 && O.ref_begin == 700 && O.score == 3 && O.cigar_len == 3);
    O = jst_rescue_record(locus(11, 720, 750), 3, 2, 1, 8, true, 725, 750, 5, 0, 3, 20, 300);  // a dovetail
    EXPECT_TRUE(O.status == SPM_RESCUE_NOT_CONCORDANT && O.tlen == 0);
    O = jst_rescue_record(locus(11, 720, 750), 3, 2, 1, 8, true, 720, 750, 5, 0, 3, 20, 300);  // the same begin: still concordant
    EXPECT_TRUE(O.status == SPM_RESCUE_RESCUED && O.tlen == 30);
    // mate 1 reverse as the anchor: mate 2 forward is rescued, tlen of mate 1 negative
    O = jst_rescue_record(locus(9, 720, 750), 3, 2, 0, 10, true, 500, 530, 0, 0, 1, 100, 300);
    EXPECT_TRUE(O.status == SPM_RESCUE_RESCUED && O.tlen == -250 && O.flag == 0xA3);
    // nothing found
    O = jst_rescue_record(locus(8, 1000, 1030), 17, 2, 0, 11, false, 0, 0, 0, 0, 0, 100, 300);
    EXPECT_TRUE(O.status == SPM_RESCUE_NONE && O.score == -1 && O.tlen == 0 && O.flag == 0x85 && O.ref_begin == 0 && O.ref_end == 0 && O.cigar_len == 0);
    O = jst_rescue_record(locus(11, 720, 750), 3, 2, 1, 8, false, 0, 0, 0, 0, 0, 100, 300);
    EXPECT_TRUE(O.status == SPM_RESCUE_NONE && O.flag == 0x65);
    // the bounds of a forward anchor are inclusive
    O = jst_rescue_record(locus(8, 1000, 1030), 0, 2, 0, 11, true, 1070, 1100, 0, 0, 1, 100, 300);
    EXPECT_TRUE(O.status == SPM_RESCUE_RESCUED && O.tlen == 100);
    O = jst_rescue_record(locus(8, 1000, 1030), 0, 2, 0, 11, true, 1270, 1300, 0, 0, 1, 100, 300);
    EXPECT_TRUE(O.status == SPM_RESCUE_RESCUED && O.tlen == 300);
}

// the plain search: the whole DP matrix column by column over [lo, last end), free begins at or right of lo
static uint64_t plain_search(const std::vector<uint8_t> &q, uint32_t sigma, uint32_t k, const std::vector<uint8_t> &text,
                             const jst_rescue_window &W)
{
    const size_t m = q.size();
    std::vector<uint32_t> col(m + 1), nxt(m + 1);
    for (size_t i = 0; i <= m; ++i)
        col[i] = (uint32_t)i;
    uint64_t best = kJstRescueNoKey;
    if (W.n_ends == 0)
        return best;
    for (uint64_t t = W.lo; t < W.e_first + W.n_ends - 1; ++t) {
        nxt[0] = 0;
        for (size_t i = 1; i <= m; ++i) {
            const bool eq = q[i - 1] < sigma && text[t] < sigma && q[i - 1] == text[t];
            nxt[i] = std::min({col[i - 1] + (eq ? 0u : 1u), col[i] + 1, nxt[i - 1] + 1});
        }
        col.swap(nxt);
        const uint64_t e = t + 1;
        if (e >= W.e_first && col[m] <= k) {
            const uint64_t key = (uint64_t)col[m] << 32 | (e - W.lo);
            best = std::min(best, key);
        }
    }
    return best;
}

static uint64_t chunked_search(const std::vector<uint8_t> &q, uint32_t sigma, uint32_t k, const std::vector<uint8_t> &text,
                               const jst_rescue_window &W)
{
    const uint32_t m = (uint32_t)q.size(), NW = (m + 63) / 64;
    std::vector<uint64_t> masks((size_t)sigma * NW);
    jst_rescue_masks(q.data(), m, sigma, NW, masks.data());
    switch (NW) {
    case 1: return jst_rescue_search<1>(masks.data(), sigma, m, k, text.data(), W);
    case 2: return jst_rescue_search<2>(masks.data(), sigma, m, k, text.data(), W);
    case 3: return jst_rescue_search<3>(masks.data(), sigma, m, k, text.data(), W);
    default: return jst_rescue_search<4>(masks.data(), sigma, m, k, text.data(), W);
    }
}

static void search_cases()
{
    std::mt19937_64 rng(20261019);
    auto below = [&](uint32_t n) { return (uint32_t)(rng() % n); };
    uint32_t found = 0, none = 0, jobs = 0, clipped = 0, long_needles = 0;
    for (int round = 0; round < 400; ++round) {
        const uint32_t sigma = round % 5 == 4 ? 5 : 4;
        const uint64_t N = 300 + below(600);
        std::vector<uint8_t> text(N);
        for (auto &c : text)
            c = (uint8_t)below(round % 7 == 3 ? 2 : 4); // (two letters: many near matches)
        const uint32_t m_choice[] = {8, 20, 33, 63, 64, 65, 100, 128, 129, 192, 200, 256};
        const uint32_t m = round < 300 ? 8 + below(40) : m_choice[round % 12];
        const uint32_t k = below(std::min(m, 9u));
        const uint32_t min_tlen = 1 + below(150), max_tlen = min_tlen + below(round % 3 ? 200 : 3);
        const bool reverse = below(2) != 0;
        const uint64_t a_begin = round % 10 == 0 ? below(40) : round % 10 == 1 ? N - 10 - below(60) : below((uint32_t)N - 40);
        const uint64_t a_end = std::min<uint64_t>(N, a_begin + 5 + below(35));
        const jst_rescue_window W = jst_rescue_window_of(a_begin, a_end, reverse, min_tlen, max_tlen, N);
        // the needle: a copy of a stretch of the window with up to k + 2 edits of every kind, or noise
        std::vector<uint8_t> q;
        if (below(8) && W.hi - W.lo > 2) {
            const uint64_t at = W.lo + below((uint32_t)(W.hi - W.lo));
            for (uint64_t t = at; q.size() < m; ++t)
                q.push_back(t < N ? text[t] : (uint8_t)below(4));
            for (uint32_t e = below(k + 3); e; --e) {
                const uint32_t at_q = below(m), kind = below(3);
                if (kind == 0)
                    q[at_q] = (uint8_t)((q[at_q] + 1 + below(3)) & 3);
                else if (kind == 1) {
                    q.erase(q.begin() + at_q);
                    q.push_back((uint8_t)below(4));
                } else {
                    q.insert(q.begin() + at_q, (uint8_t)below(4));
                    q.pop_back();
                }
            }
        } else {
            for (uint32_t i = 0; i < m; ++i)
                q.push_back((uint8_t)below(4));
        }
        if (sigma == 5)
            q[below(m)] = 4 + (uint8_t)below(3); // N, or a rank beyond sigma: neither matches anything
        if (sigma == 5 && W.hi > W.lo)
            text[W.lo + below((uint32_t)(W.hi - W.lo))] = 4; // (rank 4 on both sides is a match: ranks are compared, as everywhere)
        const uint64_t want = plain_search(q, sigma, k, text, W), got = chunked_search(q, sigma, k, text, W);
        EXPECT_TRUE(want == got);
        EXPECT_TRUE(W.lo <= W.hi && W.hi <= N && (W.n_ends == 0 || (W.e_first > W.lo && W.e_first + W.n_ends - 1 <= W.hi)));
        if (want != kJstRescueNoKey)
            EXPECT_TRUE(jst_rescue_key_d(want) <= k && W.lo + jst_rescue_key_rel(want) >= W.e_first);
        ++jobs;
        found += want != kJstRescueNoKey;
        none += want == kJstRescueNoKey;
        clipped += W.lo == 0 || W.hi == N;
        long_needles += m > 64;
    }
    std::printf("search: %u jobs, %u with a candidate, %u without, %u clipped windows, %u needles above one word\n", jobs, found, none,
                clipped, long_needles);
    EXPECT_TRUE(found >= 100 && none >= 50 && clipped >= 30 && long_needles >= 50);
}

int main()
{
    jobs_cases();
    window_cases();
    chunk_cases();
    record_cases();
    search_cases();
    std::printf("%d checks, %d failures\n", checks, failures);
    return failures != 0;
}

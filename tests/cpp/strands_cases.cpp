// strands_cases.cpp -- stranded needle sets on the host (libspm_amd/csrc/strands.hpp) without a device: the complement
// tables, the layout build_stranded hands to the ordinary create path, and its refusals.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../libspm_amd/csrc/strands.hpp"

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

// the complement by letter, written out again: the tables are by rank
static char letter_complement(char c)
{
    const char *from = "ACGTNBVDHKMRYSW", *to = "TGCANVBHDMKYRSW";
    const char *at = std::strchr(from, c);
    return at ? to[at - from] : '?';
}

static void table_cases()
{
    const struct
    {
        uint32_t sigma;
        const char *letters;
    } alphabets[] = {{4, "ACGT"}, {5, "ACGNT"}, {15, "ABCDGHKMNRSTVWY"}};
    for (const auto &A : alphabets) {
        const uint8_t *t = complement_table(A.sigma);
        EXPECT_TRUE(t != nullptr);
        if (!t)
            continue;
        std::vector<int> seen(A.sigma, 0);
        for (uint32_t r = 0; r < A.sigma; ++r) {
            EXPECT_TRUE(t[r] < A.sigma);
            EXPECT_TRUE(t[t[r]] == r); // an involution
            EXPECT_TRUE(A.letters[t[r]] == letter_complement(A.letters[r]));
            seen[t[r]] += 1;
            EXPECT_TRUE(complement_rank(t, A.sigma, (uint8_t)r) == t[r]);
        }
        for (uint32_t r = 0; r < A.sigma; ++r)
            EXPECT_TRUE(seen[r] == 1);
        for (uint32_t r = A.sigma; r < 256; ++r)
            EXPECT_TRUE(complement_rank(t, A.sigma, (uint8_t)r) == r); // matches nothing on either strand
    }
    for (uint32_t sigma = 0; sigma < 300; ++sigma)
        EXPECT_TRUE((complement_table(sigma) != nullptr) == (sigma == 4 || sigma == 5 || sigma == 15));
}

static void layout_cases()
{
    // three reads, the middle one empty, the last with a rank >= sigma; dna4
    const uint8_t ranks[] = {0, 1, 1, 3, /* */ 2, 2, 9, 0, 3};
    const uint32_t offsets[] = {0, 4, 4, 9};
    const uint16_t k[] = {1, 7, 2};
    const stranded_set S = build_stranded(ranks, offsets, 3, k, 4);
    EXPECT_TRUE(S.status == SPM_OK);
    const std::vector<uint32_t> want_off = {0, 4, 8, 8, 8, 13, 18};
    EXPECT_TRUE(S.offsets == want_off);
    const std::vector<uint8_t> want = {0, 1, 1, 3, /* rc */ 0, 2, 2, 3, /* */ 2, 2, 9, 0, 3, /* rc */ 0, 3, 9, 1, 1};
    EXPECT_TRUE(S.ranks == want);
    const std::vector<uint16_t> want_k = {1, 1, 7, 7, 2, 2};
    EXPECT_TRUE(S.k == want_k);
    // no k: none comes back
    const stranded_set N = build_stranded(ranks, offsets, 3, nullptr, 4);
    EXPECT_TRUE(N.status == SPM_OK && N.k.empty() && N.ranks == want && N.offsets == want_off);
    // offsets that do not begin at 0: the result does
    const uint32_t off2[] = {4, 9};
    const stranded_set T = build_stranded(ranks, off2, 1, k, 4);
    EXPECT_TRUE(T.status == SPM_OK && T.offsets == (std::vector<uint32_t>{0, 5, 10}));
    EXPECT_TRUE(T.ranks == (std::vector<uint8_t>{2, 2, 9, 0, 3, 0, 3, 9, 1, 1}) && T.k == (std::vector<uint16_t>{1, 1}));
    // no reads at all
    const stranded_set E = build_stranded(nullptr, nullptr, 0, nullptr, 5);
    EXPECT_TRUE(E.status == SPM_OK && E.ranks.empty() && E.offsets == std::vector<uint32_t>{0} && E.k.empty());
    // the reverse complement of the reverse complement is the read: every alphabet, random reads
    uint64_t z = 12345;
    for (uint32_t sigma : {4u, 5u, 15u})
        for (int trial = 0; trial < 50; ++trial) {
            std::vector<uint8_t> r;
            std::vector<uint32_t> off = {0};
            std::vector<uint16_t> kk;
            const uint32_t n = 1 + (uint32_t)(trial % 7);
            for (uint32_t i = 0; i < n; ++i) {
                z = z * 6364136223846793005ull + 1442695040888963407ull;
                const uint32_t m = (uint32_t)(z >> 33) % 40;
                for (uint32_t j = 0; j < m; ++j) {
                    z = z * 6364136223846793005ull + 1442695040888963407ull;
                    r.push_back((uint8_t)((z >> 33) % (sigma + 2))); // some ranks >= sigma
                }
                off.push_back((uint32_t)r.size());
                kk.push_back((uint16_t)i);
            }
            const stranded_set A = build_stranded(r.data(), off.data(), n, kk.data(), sigma);
            EXPECT_TRUE(A.status == SPM_OK && A.offsets.size() == 2 * n + 1 && A.k.size() == 2 * n && A.ranks.size() == 2 * r.size());
            if (A.status != SPM_OK)
                continue;
            const stranded_set B = build_stranded(A.ranks.data(), A.offsets.data(), 2 * n, A.k.data(), sigma);
            EXPECT_TRUE(B.status == SPM_OK);
            for (uint32_t i = 0; i < n && B.status == SPM_OK; ++i) {
                const uint32_t m = off[i + 1] - off[i];
                EXPECT_TRUE(A.offsets[2 * i + 1] - A.offsets[2 * i] == m && A.offsets[2 * i + 2] - A.offsets[2 * i + 1] == m);
                EXPECT_TRUE(A.k[2 * i] == i && A.k[2 * i + 1] == i);
                EXPECT_TRUE(m == 0 || std::memcmp(A.ranks.data() + A.offsets[2 * i], r.data() + off[i], m) == 0);
                // pattern 4i+3 of B is the reverse complement of pattern 2i+1 of A: the read again
                EXPECT_TRUE(m == 0 || std::memcmp(B.ranks.data() + B.offsets[4 * i + 3], r.data() + off[i], m) == 0);
                for (uint32_t j = 0; j < m; ++j) {
                    const uint8_t a = r[off[i] + j], b = A.ranks[A.offsets[2 * i + 1] + m - 1 - j];
                    EXPECT_TRUE(a < sigma ? b == complement_table(sigma)[a] : b == a);
                }
            }
        }
}

static void refusal_cases()
{
    const uint8_t ranks[] = {0, 1, 2, 3};
    const uint32_t offsets[] = {0, 4};
    const uint16_t k[] = {0};
    EXPECT_TRUE(build_stranded(ranks, offsets, 1, k, 6).status == SPM_E_UNSUPPORTED);
    EXPECT_TRUE(build_stranded(ranks, offsets, 1, k, 255).status == SPM_E_UNSUPPORTED);
    // twice the reads do not fit: decided from n alone -- no offsets, no ranks are read (there are none)
    EXPECT_TRUE(build_stranded(nullptr, nullptr, 0x80000000u, nullptr, 4).status == SPM_E_UNSUPPORTED);
    EXPECT_TRUE(build_stranded(nullptr, nullptr, 0xFFFFFFFFu, nullptr, 4).status == SPM_E_UNSUPPORTED);
    // twice the symbols do not fit: decided from the offsets alone -- no rank is read, nothing is allocated
    const uint32_t big[] = {0, 0x80000000u};
    stranded_set S = build_stranded(nullptr, big, 1, k, 4);
    EXPECT_TRUE(S.status == SPM_E_UNSUPPORTED && S.ranks.empty() && S.offsets.empty() && S.k.empty());
    const uint32_t big2[] = {0, 0x40000000u, 0x80000000u};
    EXPECT_TRUE(build_stranded(nullptr, big2, 2, nullptr, 4).status == SPM_E_UNSUPPORTED);
    const uint32_t fits[] = {0, 0x7FFFFFFFu}; // 2^32 - 2 symbols would fit: it is the missing symbols that are refused
    EXPECT_TRUE(build_stranded(nullptr, fits, 1, nullptr, 4).status == SPM_E_INVALID);
    const uint32_t down[] = {4, 2, 5};
    EXPECT_TRUE(build_stranded(ranks, down, 2, nullptr, 4).status == SPM_E_INVALID);
    EXPECT_TRUE(build_stranded(ranks, nullptr, 1, nullptr, 4).status == SPM_E_INVALID);
    EXPECT_TRUE(std::string(build_stranded(ranks, offsets, 1, k, 6).why).size() > 0);
}

int main()
{
    table_cases();
    layout_cases();
    refusal_cases();
    std::printf("%d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}

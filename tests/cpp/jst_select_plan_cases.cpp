// jst_select_plan_cases.cpp -- the host-side decisions of one pan-genome hit selection (plan_jst_select,
// libspm_amd/csrc/select_plan.hpp) without a device: the three fields of the sort key and their bit budget, the fields of
// zero bits, a key of exactly 64 bits, the refusals made before anything is launched, and plan_select left as it was.
#include <cstdint>
#include <cstdio>

#include "../../libspm_amd/csrc/select_plan.hpp"

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

static spm_select_opts opts(uint32_t flags, uint32_t window, uint32_t strata = 0, uint32_t reserved = 0)
{
    return spm_select_opts{flags, window, strata, reserved};
}

// the smallest count whose largest index needs exactly `bits` bits
static uint64_t count_of(uint32_t bits) { return bits ? (1ull << (bits - 1)) + 1 : 1; }
// the largest value of `bits` bits
static uint64_t max_of(uint32_t bits) { return bits >= 64 ? ~0ull : (1ull << bits) - 1; }

static void budget_cases()
{
    const spm_select_opts loci_k = opts(SPM_SELECT_LOCI, SPM_SELECT_WINDOW_K);
    // the read-mapping shape: 64 haplotypes (6 bits), 20 000 reads (15 bits), positions up to 2^22 + insertions (23 bits)
    jst_select_plan P = plan_jst_select(loci_k, 25000000, 64, 20000, (1ull << 22) + 12345, true, true, 3);
    EXPECT_TRUE(P.status == SPM_OK && P.hap_bits == 6 && P.pat_bits == 15 && P.pos_bits == 23 && P.key_bits == 44);
    // fields of zero bits
    P = plan_jst_select(loci_k, 10, 1, 20000, 1000, true, true, 3);
    EXPECT_TRUE(P.status == SPM_OK && P.hap_bits == 0 && P.pat_bits == 15 && P.pos_bits == 10 && P.key_bits == 25);
    P = plan_jst_select(loci_k, 10, 64, 1, 1000, true, true, 3);
    EXPECT_TRUE(P.status == SPM_OK && P.hap_bits == 6 && P.pat_bits == 0 && P.pos_bits == 10 && P.key_bits == 16);
    P = plan_jst_select(loci_k, 10, 1, 1, 1000, true, true, 3);
    EXPECT_TRUE(P.status == SPM_OK && P.hap_bits == 0 && P.pat_bits == 0 && P.key_bits == 10);
    P = plan_jst_select(loci_k, 10, 0, 0, 1000, true, true, 3); // (counts of 0 are counts of 1)
    EXPECT_TRUE(P.status == SPM_OK && P.hap_bits == 0 && P.pat_bits == 0 && P.key_bits == 10);
    P = plan_jst_select(loci_k, 10, 2, 2, 0, true, true, 3);
    EXPECT_TRUE(P.status == SPM_OK && P.hap_bits == 1 && P.pat_bits == 1 && P.pos_bits == 0 && P.key_bits == 2);
    P = plan_jst_select(loci_k, 0, 1, 1, 0, true, true, 3); // nothing to tell apart still sorts one bit
    EXPECT_TRUE(P.status == SPM_OK && P.key_bits == 1);
    P = plan_jst_select(loci_k, 1, 1, 1, ~0ull, true, true, 3); // the position alone fills the key
    EXPECT_TRUE(P.status == SPM_OK && P.pos_bits == 64 && P.key_bits == 64);
    // the legal extreme of the tree: 65 535 haplotypes x 100 000 needles leave 31 bits of position
    P = plan_jst_select(loci_k, 1000, 65535, 100000, max_of(31), true, true, 3);
    EXPECT_TRUE(P.status == SPM_OK && P.hap_bits == 16 && P.pat_bits == 17 && P.pos_bits == 31 && P.key_bits == 64);
    P = plan_jst_select(loci_k, 1000, 65535, 100000, max_of(31) + 1, true, true, 3);
    EXPECT_TRUE(P.status == SPM_E_UNSUPPORTED);
    // every split of the 64 bits: fits at exactly 64, refused at 65, from each of the three fields
    for (uint32_t hap_bits = 0; hap_bits <= 16; ++hap_bits)
        for (uint32_t pat_bits = 0; pat_bits <= 32; ++pat_bits) {
            const uint32_t room = 64 - hap_bits - pat_bits;
            P = plan_jst_select(loci_k, 1, count_of(hap_bits), count_of(pat_bits), max_of(room), true, true, 3);
            EXPECT_TRUE(P.status == SPM_OK && P.hap_bits == hap_bits && P.pat_bits == pat_bits && P.pos_bits == room &&
                        P.key_bits == 64);
            if (room < 64) {
                P = plan_jst_select(loci_k, 1, count_of(hap_bits), count_of(pat_bits), max_of(room) + 1, true, true, 3);
                EXPECT_TRUE(P.status == SPM_E_UNSUPPORTED);
            }
            P = plan_jst_select(loci_k, 1, count_of(hap_bits + 1), count_of(pat_bits), max_of(room), true, true, 3);
            EXPECT_TRUE(P.status == SPM_E_UNSUPPORTED);
            P = plan_jst_select(loci_k, 1, count_of(hap_bits), count_of(pat_bits + 1), max_of(room), true, true, 3);
            EXPECT_TRUE(P.status == SPM_E_UNSUPPORTED);
            P = plan_jst_select(loci_k, 1, count_of(hap_bits), count_of(pat_bits), max_of(room) >> 1, true, true, 3);
            EXPECT_TRUE(P.status == SPM_OK && P.key_bits == (room ? 63u : 64u));
        }
    // more than 2^32 - 1 records
    P = plan_jst_select(loci_k, 0xFFFFFFFFull, 64, 4, 1000, true, true, 3);
    EXPECT_TRUE(P.status == SPM_OK);
    P = plan_jst_select(loci_k, 0x100000000ull, 64, 4, 1000, true, true, 3);
    EXPECT_TRUE(P.status == SPM_E_UNSUPPORTED);
    P = plan_jst_select(opts(0, 0), 0x100000000ull, 64, 4, 1000, true, true, 3); // a sorted copy is a sort all the same
    EXPECT_TRUE(P.status == SPM_E_UNSUPPORTED);
}

static void window_cases()
{
    jst_select_plan P = plan_jst_select(opts(SPM_SELECT_LOCI, SPM_SELECT_WINDOW_K), 10, 8, 4, 1000, true, true, 6);
    EXPECT_TRUE(P.status == SPM_OK && P.loci && !P.best && !P.across && P.window == SPM_SELECT_WINDOW_K && P.max_window == 6 &&
                P.halo == 6);
    P = plan_jst_select(opts(SPM_SELECT_LOCI, SPM_SELECT_WINDOW_K), 10, 8, 4, 1000, true, true, 64); // the C5 needles
    EXPECT_TRUE(P.status == SPM_OK && P.max_window == 64 && P.halo == kSelHaloCap);
    P = plan_jst_select(opts(SPM_SELECT_LOCI, SPM_SELECT_WINDOW_K), 10, 8, 4, 1000, true, false, 5); // exact sets: k is 0
    EXPECT_TRUE(P.status == SPM_OK && P.window == 0 && P.halo == 0);
    P = plan_jst_select(opts(SPM_SELECT_LOCI | SPM_SELECT_BEST, 9, 2), 10, 8, 4, 1000, false, false, 0);
    EXPECT_TRUE(P.status == SPM_OK && P.loci && P.best && !P.across && P.window == 9 && P.max_window == 9 && P.halo == 9);
    P = plan_jst_select(opts(SPM_SELECT_LOCI | SPM_SELECT_BEST | SPM_SELECT_ACROSS, 200, 1), 10, 8, 4, 1000, false, false, 0);
    EXPECT_TRUE(P.status == SPM_OK && P.loci && P.best && P.across && P.window == 200 && P.halo == kSelHaloCap);
    P = plan_jst_select(opts(SPM_SELECT_BEST | SPM_SELECT_ACROSS, 77, 1), 10, 8, 4, 1000, true, true, 6); // no LOCI: no window
    EXPECT_TRUE(P.status == SPM_OK && !P.loci && P.best && P.across && P.window == 0 && P.halo == 0);
    P = plan_jst_select(opts(0, SPM_SELECT_WINDOW_K), 10, 8, 4, 1000, false, false, 0); // neither flag: the window is not read
    EXPECT_TRUE(P.status == SPM_OK && !P.loci && !P.best && P.halo == 0);
    for (uint32_t w = 0; w < 300; ++w) {
        P = plan_jst_select(opts(SPM_SELECT_LOCI, w), 10, 8, 4, 1000, false, false, 0);
        EXPECT_TRUE(P.status == SPM_OK && P.window == w && P.halo == (w < kSelHaloCap ? w : kSelHaloCap));
    }
}

static void refused_opts()
{
    // every SPM_E_INVALID
    EXPECT_TRUE(plan_jst_select(opts(8, 1), 10, 8, 4, 1000, true, true, 3).status == SPM_E_INVALID);
    EXPECT_TRUE(plan_jst_select(opts(0xDEADBEEFu, 1), 10, 8, 4, 1000, true, true, 3).status == SPM_E_INVALID);
    EXPECT_TRUE(plan_jst_select(opts(SPM_SELECT_LOCI, 1, 0, 1), 10, 8, 4, 1000, true, true, 3).status == SPM_E_INVALID);
    EXPECT_TRUE(plan_jst_select(opts(SPM_SELECT_ACROSS, 1), 10, 8, 4, 1000, true, true, 3).status == SPM_E_INVALID);
    EXPECT_TRUE(plan_jst_select(opts(SPM_SELECT_LOCI | SPM_SELECT_ACROSS, 1), 10, 8, 4, 1000, true, true, 3).status == SPM_E_INVALID);
    EXPECT_TRUE(plan_jst_select(opts(SPM_SELECT_LOCI, SPM_SELECT_WINDOW_K), 10, 8, 4, 1000, false, false, 0).status == SPM_E_INVALID);
    // ... which come before the refusals of size
    EXPECT_TRUE(plan_jst_select(opts(SPM_SELECT_ACROSS, 1), 0x100000000ull, 8, 4, 1000, true, true, 3).status == SPM_E_INVALID);
    EXPECT_TRUE(plan_jst_select(opts(SPM_SELECT_LOCI, 1, 0, 1), 1, 65535, 100000, ~0ull, true, true, 3).status == SPM_E_INVALID);
    // what is fine
    EXPECT_TRUE(plan_jst_select(opts(SPM_SELECT_LOCI | SPM_SELECT_BEST, 1, 0xFFFFFFFFu), 10, 8, 4, 1000, true, true, 3).status == SPM_OK);
    EXPECT_TRUE(plan_jst_select(opts(SPM_SELECT_BEST | SPM_SELECT_ACROSS, 0), 10, 8, 4, 1000, false, false, 0).status == SPM_OK);
    EXPECT_TRUE(plan_jst_select(opts(SPM_SELECT_LOCI, SPM_SELECT_WINDOW_K), 10, 8, 4, 1000, true, false, 0).status == SPM_OK);
    // plain selection is untouched: flag bit 4 is unknown to it, with and without BEST
    EXPECT_TRUE(SPM_SELECT_ACROSS == 4u);
    EXPECT_TRUE(plan_select(opts(SPM_SELECT_ACROSS, 1), 10, 4, 1000, true, true, 3).status == SPM_E_INVALID);
    EXPECT_TRUE(plan_select(opts(SPM_SELECT_BEST | SPM_SELECT_ACROSS, 1), 10, 4, 1000, true, true, 3).status == SPM_E_INVALID);
    EXPECT_TRUE(plan_select(opts(SPM_SELECT_LOCI | SPM_SELECT_BEST, 1), 10, 4, 1000, true, true, 3).status == SPM_OK);
}

int main()
{
    budget_cases();
    window_cases();
    refused_opts();
    std::printf("%d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}

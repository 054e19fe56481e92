// select_plan_cases.cpp -- the host-side decisions of one hit selection (libspm_amd/csrc/select_plan.hpp) without a device:
// the bit budget of the sort key with its two refusals, the halo staged in LDS, the window a needle gets, the opts that are
// refused outright.
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

static void bit_cases()
{
    EXPECT_TRUE(bits_for(0) == 0 && bits_for(1) == 1 && bits_for(2) == 2 && bits_for(3) == 2 && bits_for(4) == 3);
    EXPECT_TRUE(bits_for(255) == 8 && bits_for(256) == 9);
    EXPECT_TRUE(bits_for(~0ull) == 64 && bits_for(1ull << 63) == 64 && bits_for((1ull << 63) - 1) == 63);
    for (uint32_t b = 1; b < 64; ++b) {
        EXPECT_TRUE(bits_for(1ull << b) == b + 1);
        EXPECT_TRUE(bits_for((1ull << b) - 1) == b);
    }
}

static void budget_cases()
{
    const spm_select_opts loci_k = opts(SPM_SELECT_LOCI, SPM_SELECT_WINDOW_K);
    // the C4 shape: 100 000 needles (17 bits), ends up to 2^33 inclusive (34 bits)
    select_plan P = plan_select(loci_k, 406615, 100000, 1ull << 33, true, true, 3);
    EXPECT_TRUE(P.status == SPM_OK && P.pat_bits == 17 && P.pos_bits == 34 && P.key_bits == 51);
    P = plan_select(loci_k, 406615, 100000, (1ull << 33) - 1, true, true, 3);
    EXPECT_TRUE(P.status == SPM_OK && P.key_bits == 50);
    // one needle: no pattern bits; an empty position range still sorts one bit
    P = plan_select(loci_k, 10, 1, 1000, true, true, 3);
    EXPECT_TRUE(P.status == SPM_OK && P.pat_bits == 0 && P.pos_bits == 10 && P.key_bits == 10);
    P = plan_select(loci_k, 0, 1, 0, true, true, 3);
    EXPECT_TRUE(P.status == SPM_OK && P.key_bits == 1);
    // every split of the 64 bits: fits at 64, refused at 65
    for (uint32_t pat_bits = 0; pat_bits <= 32; ++pat_bits) {
        const uint64_t n_pat = pat_bits ? (1ull << (pat_bits - 1)) + 1 : 1; // needs exactly pat_bits bits
        const uint32_t room = 64 - pat_bits;
        const uint64_t max_fit = room == 64 ? ~0ull : (1ull << room) - 1;
        P = plan_select(loci_k, 1, n_pat, max_fit, true, true, 3);
        EXPECT_TRUE(P.status == SPM_OK && P.pat_bits == pat_bits && P.pos_bits == room && P.key_bits == 64);
        if (room < 64) {
            P = plan_select(loci_k, 1, n_pat, max_fit + 1, true, true, 3);
            EXPECT_TRUE(P.status == SPM_E_UNSUPPORTED);
        }
        P = plan_select(loci_k, 1, n_pat, max_fit >> 1, true, true, 3);
        EXPECT_TRUE(P.status == SPM_OK && P.key_bits == 63);
    }
    // more than 2^32 - 1 records
    P = plan_select(loci_k, 0xFFFFFFFFull, 4, 1000, true, true, 3);
    EXPECT_TRUE(P.status == SPM_OK);
    P = plan_select(loci_k, 0x100000000ull, 4, 1000, true, true, 3);
    EXPECT_TRUE(P.status == SPM_E_UNSUPPORTED);
    P = plan_select(opts(0, 0), 0x100000000ull, 4, 1000, true, true, 3); // a sorted copy is a sort all the same
    EXPECT_TRUE(P.status == SPM_E_UNSUPPORTED);
}

static void window_cases()
{
    // resolution for one needle
    EXPECT_TRUE(select_window(SPM_SELECT_WINDOW_K, true, 3) == 3);
    EXPECT_TRUE(select_window(SPM_SELECT_WINDOW_K, true, 0) == 0);
    EXPECT_TRUE(select_window(SPM_SELECT_WINDOW_K, false, 7) == 0); // exact sets ignore their k
    EXPECT_TRUE(select_window(5, true, 3) == 5 && select_window(5, false, 3) == 5 && select_window(0, true, 3) == 0);
    // the plan: per-needle windows only where they can differ
    select_plan P = plan_select(opts(SPM_SELECT_LOCI, SPM_SELECT_WINDOW_K), 10, 4, 1000, true, true, 6);
    EXPECT_TRUE(P.status == SPM_OK && P.loci && !P.best && P.window == SPM_SELECT_WINDOW_K && P.max_window == 6 && P.halo == 6);
    P = plan_select(opts(SPM_SELECT_LOCI, SPM_SELECT_WINDOW_K), 10, 4, 1000, true, true, 0);
    EXPECT_TRUE(P.status == SPM_OK && P.window == 0 && P.max_window == 0 && P.halo == 0);
    P = plan_select(opts(SPM_SELECT_LOCI, SPM_SELECT_WINDOW_K), 10, 4, 1000, true, false, 5);
    EXPECT_TRUE(P.status == SPM_OK && P.window == 0 && P.halo == 0);
    P = plan_select(opts(SPM_SELECT_LOCI | SPM_SELECT_BEST, 9, 2), 10, 4, 1000, false, false, 0);
    EXPECT_TRUE(P.status == SPM_OK && P.loci && P.best && P.window == 9 && P.max_window == 9 && P.halo == 9);
    // BEST alone / neither flag: no window at all, whatever the field holds
    P = plan_select(opts(SPM_SELECT_BEST, 77, 1), 10, 4, 1000, true, true, 6);
    EXPECT_TRUE(P.status == SPM_OK && !P.loci && P.best && P.window == 0 && P.halo == 0);
    P = plan_select(opts(0, SPM_SELECT_WINDOW_K), 10, 4, 1000, false, false, 0);
    EXPECT_TRUE(P.status == SPM_OK && !P.loci && !P.best && P.halo == 0);
    // the needles' own k without the needles
    P = plan_select(opts(SPM_SELECT_LOCI, SPM_SELECT_WINDOW_K), 10, 4, 1000, false, false, 0);
    EXPECT_TRUE(P.status == SPM_E_INVALID);
}

static void halo_cases()
{
    for (uint32_t w = 0; w < 300; ++w) {
        EXPECT_TRUE(select_halo(w) == (w < kSelHaloCap ? w : kSelHaloCap));
        EXPECT_TRUE(select_halo(w, 1) == (w ? 1u : 0u)); // a forced tiny halo
        const select_plan P = plan_select(opts(SPM_SELECT_LOCI, w), 10, 4, 1000, false, false, 0);
        EXPECT_TRUE(P.status == SPM_OK && P.halo <= kSelHaloCap && P.halo <= w && (P.halo == w || P.halo == kSelHaloCap));
    }
    EXPECT_TRUE(select_halo(64) == 32); // the C5 needle shape (k = 64): windows reach beyond the halo
    const select_plan P = plan_select(opts(SPM_SELECT_LOCI, SPM_SELECT_WINDOW_K), 10, 4, 1000, true, true, 2048);
    EXPECT_TRUE(P.halo == kSelHaloCap && P.max_window == 2048);
}

static void refused_opts()
{
    EXPECT_TRUE(plan_select(opts(4, 1), 10, 4, 1000, true, true, 3).status == SPM_E_INVALID);
    EXPECT_TRUE(plan_select(opts(0xDEADBEEFu, 1), 10, 4, 1000, true, true, 3).status == SPM_E_INVALID);
    EXPECT_TRUE(plan_select(opts(SPM_SELECT_LOCI, 1, 0, 1), 10, 4, 1000, true, true, 3).status == SPM_E_INVALID);
    EXPECT_TRUE(plan_select(opts(SPM_SELECT_LOCI | SPM_SELECT_BEST, 1, 0xFFFFFFFFu), 10, 4, 1000, true, true, 3).status == SPM_OK);
}

int main()
{
    bit_cases();
    budget_cases();
    window_cases();
    halo_cases();
    refused_opts();
    std::printf("%d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}

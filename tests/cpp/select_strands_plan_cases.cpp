// select_strands_plan_cases.cpp -- what SPM_SELECT_STRANDS changes in the host-side plans of a selection
// (libspm_amd/csrc/select_plan.hpp), without a device: the flag needs BEST, both kinds of selection take it, the plain one
// still refuses SPM_SELECT_ACROSS, and the minima table is sized per read.
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

static spm_select_opts opts(uint32_t flags, uint32_t window = 1, uint32_t strata = 0, uint32_t reserved = 0)
{
    return spm_select_opts{flags, window, strata, reserved};
}

static void flag_cases()
{
    static_assert(SPM_SELECT_STRANDS == 8u && SPM_SELECT_ACROSS == 4u, "spm_hip.h");
    const uint32_t L = SPM_SELECT_LOCI, B = SPM_SELECT_BEST, A = SPM_SELECT_ACROSS, S = SPM_SELECT_STRANDS;
    for (uint32_t f = 0; f < 32; ++f) {
        const select_plan P = plan_select(opts(f), 10, 6, 1000, true, true, 3);
        const bool ok = !(f & ~(L | B | S)) && (!(f & S) || (f & B));
        EXPECT_TRUE((P.status == SPM_OK) == ok);
        if (!ok)
            EXPECT_TRUE(P.status == SPM_E_INVALID && P.why[0] != 0);
        else
            EXPECT_TRUE(P.strands == ((f & S) != 0) && P.best == ((f & B) != 0) && P.loci == ((f & L) != 0));
        const jst_select_plan J = plan_jst_select(opts(f), 10, 4, 6, 1000, true, true, 3);
        const bool jok = !(f & ~(L | B | A | S)) && (!(f & S) || (f & B)) && (!(f & A) || (f & B));
        EXPECT_TRUE((J.status == SPM_OK) == jok);
        if (!jok)
            EXPECT_TRUE(J.status == SPM_E_INVALID && J.why[0] != 0);
        else
            EXPECT_TRUE(J.strands == ((f & S) != 0) && J.across == ((f & A) != 0));
    }
    EXPECT_TRUE(plan_select(opts(S), 10, 6, 1000, true, true, 3).status == SPM_E_INVALID);          // STRANDS alone
    EXPECT_TRUE(plan_select(opts(S | L), 10, 6, 1000, true, true, 3).status == SPM_E_INVALID);
    EXPECT_TRUE(plan_select(opts(S | B), 10, 6, 1000, true, true, 3).status == SPM_OK);
    EXPECT_TRUE(plan_select(opts(S | B | A), 10, 6, 1000, true, true, 3).status == SPM_E_INVALID);  // bit 4 is still refused
    EXPECT_TRUE(plan_select(opts(A | B), 10, 6, 1000, true, true, 3).status == SPM_E_INVALID);
    EXPECT_TRUE(plan_select(opts(S | B, 1, 0, 1), 10, 6, 1000, true, true, 3).status == SPM_E_INVALID);
    EXPECT_TRUE(plan_jst_select(opts(S | B | A), 10, 4, 6, 1000, true, true, 3).status == SPM_OK);
    EXPECT_TRUE(plan_jst_select(opts(S | A), 10, 4, 6, 1000, true, true, 3).status == SPM_E_INVALID);
}

static void minima_cases()
{
    const uint32_t B = SPM_SELECT_BEST, A = SPM_SELECT_ACROSS, S = SPM_SELECT_STRANDS;
    for (uint64_t n = 0; n < 70; ++n) {
        const uint64_t pats = n ? n : 1;
        EXPECT_TRUE(select_minima_slots(n, false) == pats);
        EXPECT_TRUE(select_minima_slots(n, true) == ((pats - 1) >> 1) + 1); // a raw buffer: (max_pattern >> 1) + 1
        EXPECT_TRUE(select_minima_slots(n, true) == (pats + 1) / 2);
        for (uint64_t p = 0; p < pats; ++p)
            EXPECT_TRUE((p >> 1) < select_minima_slots(n, true)); // every read has its slot
        EXPECT_TRUE(plan_select(opts(B), 10, n, 1000, true, true, 3).min_slots == pats);
        EXPECT_TRUE(plan_select(opts(B | S), 10, n, 1000, true, true, 3).min_slots == (pats + 1) / 2);
        EXPECT_TRUE(plan_select(opts(0), 10, n, 1000, true, true, 3).min_slots == 0);
        EXPECT_TRUE(plan_jst_select(opts(B | A), 10, 4, n, 1000, true, true, 3).min_slots == pats);
        EXPECT_TRUE(plan_jst_select(opts(B | A | S), 10, 4, n, 1000, true, true, 3).min_slots == (pats + 1) / 2);
        EXPECT_TRUE(plan_jst_select(opts(B | S), 37, 4, n, 1000, true, true, 3).min_slots == 37); // numbered groups: <= records
        EXPECT_TRUE(plan_jst_select(opts(B), 37, 4, n, 1000, true, true, 3).min_slots == 37);
        EXPECT_TRUE(plan_jst_select(opts(0), 37, 4, n, 1000, true, true, 3).min_slots == 0);
    }
    EXPECT_TRUE(select_minima_slots(0x100000000ull, true) == 0x80000000ull);
}

static void key_cases()
{
    const uint32_t B = SPM_SELECT_BEST, S = SPM_SELECT_STRANDS;
    // the flag changes no key of the plain selection
    for (uint64_t n : {1ull, 2ull, 3ull, 100000ull}) {
        const select_plan P0 = plan_select(opts(B), 10, n, 1000, true, true, 3), P1 = plan_select(opts(B | S), 10, n, 1000, true, true, 3);
        EXPECT_TRUE(P0.pat_bits == P1.pat_bits && P0.pos_bits == P1.pos_bits && P0.key_bits == P1.key_bits && P0.halo == P1.halo);
    }
    // pan-genome: the strand is the lowest bit of the group (haplotype << pat_bits | pattern), so it must be a pattern bit
    jst_select_plan J = plan_jst_select(opts(B | S), 10, 4, 1, 1000, true, true, 3);
    EXPECT_TRUE(J.status == SPM_OK && J.pat_bits == 1 && J.hap_bits == 2 && J.key_bits == 2 + 1 + 10);
    J = plan_jst_select(opts(B), 10, 4, 1, 1000, true, true, 3);
    EXPECT_TRUE(J.status == SPM_OK && J.pat_bits == 0 && J.key_bits == 2 + 0 + 10);
    for (uint64_t n : {2ull, 3ull, 100000ull}) {
        const jst_select_plan J0 = plan_jst_select(opts(B), 10, 4, n, 1000, true, true, 3),
                              J1 = plan_jst_select(opts(B | S), 10, 4, n, 1000, true, true, 3);
        EXPECT_TRUE(J0.pat_bits == J1.pat_bits && J0.key_bits == J1.key_bits);
    }
}

int main()
{
    flag_cases();
    minima_cases();
    key_cases();
    std::printf("%d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}

// jst_locate_plan_cases.cpp -- the host-side plan of spm_hip_jst_selection_align (plan_jst_locate,
// libspm_amd/csrc/select_plan.hpp): the widths of the sort key and what is refused before any launch.  No device.
#include <cstdio>

#include "../../libspm_amd/csrc/select_plan.hpp"

static int failures = 0, checks = 0;
#define EXPECT_TRUE(cond)                                                                                              \
    do {                                                                                                               \
        ++checks;                                                                                                      \
        if (!(cond)) {                                                                                                 \
            ++failures;                                                                                                \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);                                              \
        }                                                                                                              \
    } while (0)

int main()
{
    using spm_hip::plan_jst_locate;
    // worked by hand: one needle needs no pattern bit; a position may equal the buffer's length (an exclusive end)
    EXPECT_TRUE(plan_jst_locate(10, 1, 255).ctx_bits == 8 && plan_jst_locate(10, 1, 256).ctx_bits == 9);
    EXPECT_TRUE(plan_jst_locate(10, 1, 256).pat_bits == 0 && plan_jst_locate(10, 2, 256).pat_bits == 1);
    EXPECT_TRUE(plan_jst_locate(10, 20000, 1000000).key_bits == 15 + 20);
    EXPECT_TRUE(plan_jst_locate(0, 0, 0).status == SPM_OK && plan_jst_locate(0, 0, 0).key_bits == 1);
    EXPECT_TRUE(plan_jst_locate(0xFFFFFFFFull, 1, 1).status == SPM_OK);
    EXPECT_TRUE(plan_jst_locate(0x100000000ull, 1, 1).status == SPM_E_UNSUPPORTED);
    // every split of the 64 bits, and one bit more
    for (unsigned pb = 0; pb <= 32; ++pb)
        for (unsigned cb = 0; cb <= 64; ++cb) {
            std::uint64_t const n_patterns = pb == 0 ? 1 : (1ull << (pb - 1)) + 1;   // needs exactly pb bits
            std::uint64_t const ctx = cb == 0 ? 0 : cb == 64 ? ~0ull : (1ull << (cb - 1)) + (cb > 1);
            auto const P = plan_jst_locate(5, n_patterns, ctx);
            EXPECT_TRUE(P.pat_bits == pb && P.ctx_bits == cb);
            EXPECT_TRUE((P.status == SPM_OK) == (pb + cb <= 64));
            if (P.status == SPM_OK)
                EXPECT_TRUE(P.key_bits == (pb + cb ? pb + cb : 1u) && P.key_bits <= 64);
            else
                EXPECT_TRUE(P.why[0] != 0);
        }
    std::printf("%d checks, %d failures\n", checks, failures);
    return failures;
}

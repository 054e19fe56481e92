// index_plan_cases.cpp -- the pure decisions of the seed index planner (libspm_amd/csrc/index_build.hpp) on rows worked out
// by hand: key length and largest stride from the shortest seed, the stride cost model, and when the dense pass is wanted.
#include <cstdint>
#include <cstdio>

#include "index_build.hpp"

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

static bool plan_is(const key_plan &K, bool ok, uint32_t H, uint32_t Smax) { return K.ok == ok && K.H == H && K.Smax == Smax; }

static void key_and_stride()
{
    const index_tuning T;
    EXPECT_TRUE(!choose_key_and_stride(8, 100, T).ok); // shorter than the shortest key
    for (uint32_t q = 9; q <= 12; ++q) // the whole seed is the key
        EXPECT_TRUE(plan_is(choose_key_and_stride(q, 100, T), true, q, 1));
    for (uint32_t q = 13; q <= 16; ++q) // one symbol of key given up for stride 2
        EXPECT_TRUE(plan_is(choose_key_and_stride(q, 100, T), true, q - 1, 2));
    // full keys: the largest power of two <= q - 15, at most 16
    EXPECT_TRUE(plan_is(choose_key_and_stride(17, 100, T), true, 16, 2));
    EXPECT_TRUE(plan_is(choose_key_and_stride(18, 100, T), true, 16, 2));
    EXPECT_TRUE(plan_is(choose_key_and_stride(19, 100, T), true, 16, 4));
    EXPECT_TRUE(plan_is(choose_key_and_stride(25, 100, T), true, 16, 8));
    EXPECT_TRUE(plan_is(choose_key_and_stride(31, 100, T), true, 16, 16));
    EXPECT_TRUE(plan_is(choose_key_and_stride(32, 100, T), true, 16, 16));
    EXPECT_TRUE(plan_is(choose_key_and_stride(37, 100, T), true, 16, 16));
    // 4^9 = 262 144 keys of 9 symbols: 20 000 seeds are 7.6 % of them, 21 000 are 8.01 % (the limit is 8 %)
    EXPECT_TRUE(plan_is(choose_key_and_stride(9, 20000, T), true, 9, 1));
    EXPECT_TRUE(!choose_key_and_stride(9, 21000, T).ok);
    EXPECT_TRUE(!choose_key_and_stride(9, 60000, T).ok);
    EXPECT_TRUE(choose_key_and_stride(10, 60000, T).ok); // 4^10: 5.7 %
    index_tuning F = T;
    F.force_stride = 1;
    EXPECT_TRUE(plan_is(choose_key_and_stride(37, 100, F), true, 16, 1));
    F.force_stride = 4;
    EXPECT_TRUE(plan_is(choose_key_and_stride(37, 100, F), true, 16, 4));
    EXPECT_TRUE(plan_is(choose_key_and_stride(17, 100, F), true, 16, 2)); // (a stride the seeds do not allow is not forced)
    F.force_stride = 32;
    EXPECT_TRUE(plan_is(choose_key_and_stride(37, 100, F), true, 16, 16));
}

static bool stride_is(const stride_choice &c, uint32_t stride, uint64_t passes) { return c.stride == stride && c.passes == passes; }

static void strides()
{
    // cost = passes x (1 + 0.3 x (Smax / s - 1))
    // 24 000 seeds, Smax 16, 57 344 keys per pass: s = 16: 7 x 1 = 7; 8: 4 x 1.3 = 5.2; 4: 2 x 1.9 = 3.8; 2: 1 x 3.1; 1: 1 x 5.5
    EXPECT_TRUE(stride_is(best_stride(24000, 16, 57344), 2, 1));
    // 80 000 seeds: s = 16: 23; 8: 12 x 1.3 = 15.6; 4: 6 x 1.9 = 11.4; 2: 3 x 3.1 = 9.3; 1: 2 x 5.5 = 11
    EXPECT_TRUE(stride_is(best_stride(80000, 16, 57344), 2, 3));
    // 400 000 seeds: s = 1: 7 x 5.5 = 38.5; 2: 14 x 3.1 = 43.4
    EXPECT_TRUE(stride_is(best_stride(400000, 16, 57344), 1, 7));
    // one pass at the largest stride: nothing beats cost 1
    EXPECT_TRUE(stride_is(best_stride(4096, 8, 57344), 8, 1));
    EXPECT_TRUE(stride_is(best_stride(1, 16, 1024), 16, 1));
    // 2 400 seeds, Smax 2, 1 024 keys per pass: s = 2: 5 x 1 = 5; 1: 3 x 1.3 = 3.9
    EXPECT_TRUE(stride_is(best_stride(2400, 2, 1024), 1, 3));
    // 2 048 seeds, Smax 2, 2 048 keys per pass: s = 2: 2 x 1 = 2; 1: 1 x 1.3
    EXPECT_TRUE(stride_is(best_stride(2048, 2, 2048), 1, 1));
    EXPECT_TRUE(stride_is(best_stride(100, 1, 57344), 1, 1));
}

static void dense_or_not()
{
    const uint8_t ranks[150] = {0};
    const uint32_t offsets[2] = {0, 150};
    int32_t m = 150, k = 3;
    needle_view nv;
    nv.algo = SPM_ALGO_MYERS;
    nv.n = 1;
    nv.ranks = ranks;
    nv.offsets = offsets;
    nv.m = &m;
    nv.k = &k;
    nv.max_k = 3;
    index_tuning T;
    key_plan K;
    K.ok = true;
    K.Smax = 16;
    EXPECT_TRUE(!wants_dense_pass(nv, T, K, 24000)); // one pass at stride 2
    EXPECT_TRUE(wants_dense_pass(nv, T, K, 80000));  // three passes
    K.Smax = 1;
    EXPECT_TRUE(wants_dense_pass(nv, T, K, 100));    // stride 1
    K.Smax = 16;
    EXPECT_TRUE(wants_dense_pass(nv, T, key_plan(), 100)); // no sparse plan
    T.dense = 0;
    EXPECT_TRUE(!wants_dense_pass(nv, T, K, 80000));
    T.dense = 2;
    EXPECT_TRUE(wants_dense_pass(nv, T, K, 100));
    m = 63; // k + 1 keys of 16 symbols do not fit
    EXPECT_TRUE(!wants_dense_pass(nv, T, K, 100));
    m = 150;
    nv.sigma = 5;
    EXPECT_TRUE(!wants_dense_pass(nv, T, K, 100));
    nv.sigma = 4;
    nv.max_k = k = 8; // band-merging sets keep their sparse passes
    EXPECT_TRUE(!wants_dense_pass(nv, T, K, 100));
}

int main()
{
    key_and_stride();
    strides();
    dense_or_not();
    std::printf("%d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}

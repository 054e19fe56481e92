// jst_collapse_core_cases.cpp -- the order and equality rule of the collapse (libspm_amd/csrc/jst_collapse_core.hpp) on the
// host: the same templates the walk kernels instantiate.  A program of its own (plain g++, and g++ -fsanitize=address,undefined).
//   * the tuple order, field by field;
//   * equal tuples whose words differ in the first, a middle or the last word;
//   * a transcript that is a prefix of another (decided by cigar_len, before any word is read);
//   * the in-group ranking against a sort of the same items with the same rule; the key plan.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "jst_collapse_core.hpp"

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

struct item
{
    jst_locus_key k;
    std::vector<uint32_t> w; // exactly k.cigar_len words: a read past them is what the sanitizer build is for
};

static item make(uint32_t pattern, uint64_t b, uint64_t e, int32_t score, std::vector<uint32_t> w)
{
    item x;
    x.k.pattern = pattern;
    x.k.ref_begin = b;
    x.k.ref_end = e;
    x.k.ref_score = score;
    x.k.cigar_len = static_cast<uint32_t>(w.size());
    x.w = std::move(w);
    return x;
}

static int cmp(item const & a, item const & b) { return jst_collapse_cmp(a.k, a.w.data(), b.k, b.w.data()); }

struct view
{
    std::vector<item> const & v;
    jst_locus_key key(uint32_t j) const { return v[j].k; }
    uint32_t const * words(uint32_t j) const { return v[j].w.data(); }
};

static constexpr uint32_t EQ = 7, X = 8, I = 1, D = 2;
static uint32_t op(uint32_t n, uint32_t o) { return n << 4 | o; }

static void order_cases()
{
    item const base = make(3, 100, 140, 1, {op(20, EQ), op(1, X), op(19, EQ)});
    // every field of the tuple, in its place in the order: an earlier field wins against all later ones
    item a = base, b = base;
    a.k.pattern = 2, a.k.ref_begin = 900;
    EXPECT_TRUE(cmp(a, base) < 0 && cmp(base, a) > 0);
    a = base, a.k.ref_begin = 99, a.k.ref_end = 900;
    EXPECT_TRUE(cmp(a, base) < 0 && cmp(base, a) > 0);
    a = base, a.k.ref_end = 139, a.k.ref_score = 9;
    EXPECT_TRUE(cmp(a, base) < 0 && cmp(base, a) > 0);
    a = base, a.k.ref_score = 0, a.w[0] = op(900, EQ);
    EXPECT_TRUE(cmp(a, base) < 0 && cmp(base, a) > 0);
    a = base, a.k.ref_score = -1; // signed
    EXPECT_TRUE(cmp(a, base) < 0);
    a = base, a.k.ref_begin = 1ull << 40, b = base, b.k.ref_begin = (1ull << 40) + 1; // 64 bits
    EXPECT_TRUE(cmp(a, b) < 0);
    EXPECT_TRUE(cmp(base, base) == 0);
    // equal tuples: the first, a middle, the last word decides
    for (size_t at = 0; at < 3; ++at) {
        a = base, b = base;
        b.w[at] += 16;
        EXPECT_TRUE(cmp(a, b) < 0 && cmp(b, a) > 0);
        for (size_t later = at + 1; later < 3; ++later) { // a later word cannot turn it round
            item c = a;
            c.w[later] = 0xFFFFFFFFu;
            EXPECT_TRUE(cmp(c, b) < 0);
        }
    }
    // words are compared as uint32: the top bit set is large, not negative
    a = base, b = base, a.w[1] = 0x7FFFFFFFu, b.w[1] = 0x80000000u;
    EXPECT_TRUE(cmp(a, b) < 0);
    // the header's first worked case: 5=1D8= before 8=1D5=
    a = make(0, 2, 16, 1, {op(5, EQ), op(1, D), op(8, EQ)}), b = make(0, 2, 16, 1, {op(8, EQ), op(1, D), op(5, EQ)});
    EXPECT_TRUE(cmp(a, b) < 0);
    // a prefix: the shorter transcript is the smaller one whatever the words say, and no word past its end is read
    a = make(3, 100, 140, 1, {op(40, EQ)}), b = make(3, 100, 140, 1, {op(40, EQ), op(1, I)});
    EXPECT_TRUE(cmp(a, b) < 0 && cmp(b, a) > 0);
    a = make(3, 100, 140, 1, {op(900, EQ)});
    EXPECT_TRUE(cmp(a, b) < 0 && cmp(b, a) > 0);
    a = make(3, 100, 100, 5, {}), b = make(3, 100, 100, 5, {});
    EXPECT_TRUE(cmp(a, b) == 0); // (no words at all)
}

static uint64_t mix(uint64_t & s)
{
    s += 0x9E3779B97F4A7C15ull;
    uint64_t z = s;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// groups of random items over few distinct values, so that equal contents, equal tuples and prefixes all occur
static void rank_cases()
{
    uint64_t s = 0xC011A95Eull;
    size_t n_equal = 0, n_tuple_only = 0, n_groups = 0;
    for (int round = 0; round < 400; ++round) {
        std::vector<item> v;
        size_t const pre = mix(s) % 4, n = 1 + mix(s) % 70, post = mix(s) % 4;
        for (size_t i = 0; i < pre + n + post; ++i) {
            std::vector<uint32_t> w(1 + mix(s) % 3);
            for (uint32_t & x : w)
                x = op(1 + static_cast<uint32_t>(mix(s) % 2), mix(s) % 2 ? EQ : X);
            v.push_back(make(0, 50, 50 + mix(s) % 2, static_cast<int32_t>(mix(s) % 2), std::move(w)));
        }
        uint32_t const lo = static_cast<uint32_t>(pre), hi = static_cast<uint32_t>(pre + n);
        view const V{v};
        std::vector<uint32_t> order;
        for (uint32_t i = lo; i < hi; ++i)
            order.push_back(i);
        std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return cmp(v[x], v[y]) < 0; });
        for (uint32_t i = lo; i < hi; ++i) {
            jst_collapse_rank_result const R = jst_collapse_rank(V, lo, hi, i);
            uint32_t smaller = 0, equal = 0, tuple = 0, first = i;
            for (uint32_t j = lo; j < hi; ++j) {
                int const c = cmp(v[j], v[i]);
                smaller += c < 0;
                equal += c == 0;
                tuple += jst_collapse_cmp_tuple(v[j].k, v[i].k) == 0;
                if (c == 0 && j < first)
                    first = j;
            }
            EXPECT_TRUE(R.smaller == smaller && R.n_equal == equal && R.n_tuple == tuple && R.first == first);
            EXPECT_TRUE(R.first >= lo && R.first <= i && R.n_equal >= 1 && R.n_tuple >= R.n_equal);
            // the rank is the position of the first equal item in the sorted group
            EXPECT_TRUE(cmp(v[order[R.smaller]], v[i]) == 0 && (R.smaller == 0 || cmp(v[order[R.smaller - 1]], v[i]) < 0));
            n_equal += R.n_equal > 1;
            n_tuple_only += R.n_tuple > R.n_equal;
        }
        ++n_groups;
    }
    EXPECT_TRUE(n_equal > 100 && n_tuple_only > 100 && n_groups == 400);
    // a group of one, at either end of the view
    std::vector<item> v{make(0, 1, 2, 0, {op(1, EQ)}), make(0, 1, 2, 0, {op(1, EQ)})};
    view const V{v};
    jst_collapse_rank_result R = jst_collapse_rank(V, 0, 1, 0);
    EXPECT_TRUE(R.smaller == 0 && R.first == 0 && R.n_equal == 1 && R.n_tuple == 1);
    R = jst_collapse_rank(V, 1, 2, 1);
    EXPECT_TRUE(R.smaller == 0 && R.first == 1 && R.n_equal == 1);
    R = jst_collapse_rank(V, 0, 2, 1);
    EXPECT_TRUE(R.smaller == 0 && R.first == 0 && R.n_equal == 2);
}

static void plan_cases()
{
    EXPECT_TRUE(jst_collapse_bits(0) == 0 && jst_collapse_bits(1) == 1 && jst_collapse_bits(255) == 8 && jst_collapse_bits(256) == 9);
    EXPECT_TRUE(jst_collapse_bits(~0ull) == 64);
    jst_collapse_plan p = plan_jst_collapse(1, 16000);
    EXPECT_TRUE(p.ok && p.pat_bits == 0 && p.ref_bits == 14);
    p = plan_jst_collapse(0, 0);
    EXPECT_TRUE(p.ok && p.pat_bits == 0 && p.ref_bits == 0);
    p = plan_jst_collapse(1u << 20, (1ull << 44) - 1);
    EXPECT_TRUE(p.ok && p.pat_bits == 20 && p.ref_bits == 44);
    p = plan_jst_collapse(1u << 20, 1ull << 44); // the length itself must fit: an anchor may equal it
    EXPECT_TRUE(!p.ok && p.ref_bits == 45);
    p = plan_jst_collapse((1u << 20) + 1, (1ull << 44) - 1);
    EXPECT_TRUE(!p.ok && p.pat_bits == 21);
    p = plan_jst_collapse(1, ~0ull);
    EXPECT_TRUE(p.ok && p.ref_bits == 64);
}

int main()
{
    order_cases();
    rank_cases();
    plan_cases();
    std::printf("%d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}

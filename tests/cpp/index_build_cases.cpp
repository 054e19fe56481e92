// index_build_cases.cpp -- the seed index build (libspm_amd/csrc/index_build.hpp) pinned bit for bit, without a device:
// needle sets from a fixed integer generator, explicit tuning (the environment is never read), every set built with 1
// and with 4 threads, and per build one line with the plan (return code, passes, stride, key length, anchored, dense,
// hash variant of the first pass) and a 64-bit FNV-1a digest over every field and vector of the seed_index and of each
// filter_index.  tests/golden/index_build/digests.txt holds the lines of the commit named there;
// tests/test_index_build_cpp.py compares.  The program uses only what the index build promises to keep:
// build_filter_index(nv, T, X), index_tuning, needle_view, filter_index, seed_index.
//
//   index_build_cases          the cases
//   index_build_cases --time   build time of the two 100 000-needle sets (dense pass; seven anchored passes), 16 threads
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "index_build.hpp"

using namespace spm_hip;

namespace
{

struct generator // xorshift64*
{
    uint64_t s;
    explicit generator(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 0x1234567ull) {}
    uint64_t next()
    {
        s ^= s >> 12;
        s ^= s << 25;
        s ^= s >> 27;
        return s * 0x2545F4914F6CDD1Dull;
    }
    uint32_t below(uint32_t n) { return (uint32_t)((next() >> 33) % n); }
};

using needle = std::vector<uint8_t>;

needle random_needle(generator &g, uint32_t m, const std::vector<uint8_t> &alphabet = {0, 1, 2, 3})
{
    needle x(m);
    for (uint8_t &c : x)
        c = alphabet[g.below((uint32_t)alphabet.size())];
    return x;
}

std::vector<needle> random_set(uint64_t seed, uint32_t n, uint32_t m, const std::vector<uint8_t> &alphabet = {0, 1, 2, 3})
{
    generator g(seed);
    std::vector<needle> r;
    for (uint32_t i = 0; i < n; ++i)
        r.push_back(random_needle(g, m, alphabet));
    return r;
}

needle repeat_of(const std::vector<uint8_t> &unit, uint32_t m)
{
    needle x(m);
    for (uint32_t i = 0; i < m; ++i)
        x[i] = unit[i % unit.size()];
    return x;
}

struct index_case
{
    std::string name;
    int algo = SPM_ALGO_MYERS;
    uint32_t sigma = 4;
    std::vector<needle> needles;
    uint32_t k = 3;
    index_tuning T;
};

struct flat_set // a needle set as needle_view wants it
{
    std::vector<uint8_t> ranks;
    std::vector<uint32_t> offsets;
    std::vector<int32_t> m, k;
    needle_view nv;
    flat_set(const index_case &c)
    {
        offsets.push_back(0);
        for (const needle &x : c.needles) {
            ranks.insert(ranks.end(), x.begin(), x.end());
            offsets.push_back((uint32_t)ranks.size());
            m.push_back((int32_t)x.size());
            k.push_back(c.algo == SPM_ALGO_MYERS ? (int32_t)c.k : 0);
        }
        nv.algo = c.algo;
        nv.n = (uint32_t)c.needles.size();
        nv.sigma = c.sigma;
        nv.ranks = ranks.data();
        nv.offsets = offsets.data();
        nv.m = m.data();
        nv.k = k.data();
        nv.max_k = c.algo == SPM_ALGO_MYERS ? c.k : 0;
    }
};

struct fnv1a
{
    uint64_t h = 0xCBF29CE484222325ull;
    void u64(uint64_t v)
    {
        for (int i = 0; i < 8; ++i) {
            h ^= (v >> (8 * i)) & 0xFF;
            h *= 0x100000001B3ull;
        }
    }
    template <typename T>
    void ints(const std::vector<T> &v)
    {
        u64(v.size());
        for (const T &x : v)
            u64((uint64_t)x);
    }
    void quads(const std::vector<u32x4> &v)
    {
        u64(v.size());
        for (const u32x4 &q : v) {
            u64(q.x);
            u64(q.y);
            u64(q.z);
            u64(q.w);
        }
    }
};

uint64_t digest(const seed_index &X)
{
    fnv1a d;
    d.u64(X.fidx.size());
    d.u64(X.filter_stride);
    d.u64(X.filter_key_len);
    d.u64(X.filter_anchored);
    d.u64(X.filter_dense);
    d.u64(X.filter_max_range);
    d.ints(X.seed_q);
    d.ints(X.seed_n);
    d.ints(X.seed_off);
    d.ints(X.seed_len);
    d.ints(X.seed_c);
    d.ints(X.seed_first);
    d.quads(X.h_entries);
    for (const filter_index &F : X.fidx) {
        d.u64(F.anchor_c);
        d.u64(F.anchor_cm);
        d.u64(F.ok);
        d.u64(F.dense);
        d.u64(F.n_pat);
        for (uint32_t i = 0; i < kDensePatterns; ++i) {
            d.u64(F.pat_c[i]);
            d.u64(F.pat_cm[i]);
        }
        d.u64(F.dimer_set);
        d.u64(F.bucket_shift);
        d.u64(F.stride);
        d.u64(F.key_len);
        d.u64(F.bitmap_words);
        d.u64(F.n_probes);
        d.u64(F.hash_variant);
        d.u64(F.lds_words);
        d.u64(F.chd_slot_mask);
        d.u64(F.chd_bucket_shift);
        d.u64(F.chd_disp_off);
        d.u64(F.ht_mask);
        d.u64(F.n_keys);
        d.u64(F.n_entries);
        d.u64(F.max_range);
        d.ints(F.h_image);
        d.quads(F.h_ht);
        d.ints(F.h_buckets);
    }
    return d.h;
}

index_case make(const char *name, std::vector<needle> needles, uint32_t k)
{
    index_case c;
    c.name = name;
    c.needles = std::move(needles);
    c.k = k;
    return c;
}

std::vector<needle> with_repeats(std::vector<needle> set, uint32_t m) // a homopolymer and an (AC)n needle among the others
{
    set[set.size() / 3] = repeat_of({0}, m);
    set[2 * set.size() / 3] = repeat_of({0, 1}, m);
    return set;
}

std::vector<index_case> all_cases()
{
    std::vector<index_case> r;
    index_case c;
    // ---- the planner's branches ----
    r.push_back(make("c3_shape", random_set(1, 64, 100), 3));
    r.push_back(make("stride2_short_seeds", random_set(2, 64, 60), 3));
    r.push_back(make("k64_band_merging", random_set(3, 8, 1024), 64));
    r.push_back(make("no_filter", random_set(4, 4, 32), 3));
    c = make("sub_batches", random_set(5, 600, 150), 3);
    c.T.max_keys = 1024;
    c.T.dense = 0;
    r.push_back(c);
    c = make("anchored", random_set(31, 2000, 150), 3);
    c.T.max_keys = 4096;
    c.T.dense = 0;
    c.T.force_stride = 1;
    r.push_back(c);
    c = make("anchored_table_fails", random_set(7, 600, 150), 3);
    c.T.max_keys = 1024;
    c.T.dense = 0;
    c.T.force_stride = 1;
    r.push_back(c);
    c = make("overfull_table", random_set(8, 2000, 128), 3);
    c.T.max_keys = 65536;
    r.push_back(c);
    c = make("bloom_cascade", random_set(9, 256, 100), 3);
    c.T.hash = 1;
    r.push_back(c);
    c = make("dense_by_default", random_set(10, 600, 150), 3);
    c.T.max_keys = 1024;
    r.push_back(c);
    c = make("dense_forced_64", random_set(11, 300, 64), 3);
    c.T.dense = 2;
    r.push_back(c);
    c = make("dense_forced_100", random_set(12, 300, 100), 3);
    c.T.dense = 2;
    r.push_back(c);
    // ---- further shapes: the golden file records what they do ----
    c = make("shiftor_32", random_set(13, 256, 32), 0);
    c.algo = SPM_ALGO_SHIFTOR;
    r.push_back(c);
    r.push_back(make("whole_seed_keys", random_set(14, 100, 44), 3));
    r.push_back(make("too_dense_short_keys", random_set(15, 20000, 27), 2));
    {
        // dna5 (A0 C1 G2 N3 T4) with Ns where tests/test_host_index.py puts them
        std::vector<needle> set = random_set(27, 256, 100, {0, 1, 2, 4});
        set[7][50] = 3;
        for (uint32_t i : {0u, 31u, 62u, 99u})
            set[8][i] = 3;
        for (uint32_t i = 10; i < 20; ++i)
            set[9][i] = 3;
        c = make("dna5_with_n", set, 3);
        c.sigma = 5;
        r.push_back(c);
        for (uint32_t i = 0; i < 100; i += 8)
            set[10][i] = 3; // no stretch of 12 key symbols left
        c = make("dna5_needle_without_seeds", set, 3);
        c.sigma = 5;
        r.push_back(c);
        c = make("dna5_bloom_cascade", random_set(27, 256, 100, {0, 1, 2, 4}), 3);
        c.sigma = 5;
        c.T.hash = 1; // (the dna5 kernel reads the fingerprint table only: no passes)
        r.push_back(c);
        c = make("dna5_table_fails", random_set(16, 256, 100, {0, 1, 2, 4}), 3); // (two keys that no displacement separates)
        c.sigma = 5;
        r.push_back(c);
    }
    {
        std::vector<needle> set = random_set(17, 64, 100, {0, 2, 4, 11});
        set[3][40] = 8;
        set[4][5] = 14;
        c = make("dna15", set, 3);
        c.sigma = 15;
        r.push_back(c);
    }
    r.push_back(make("repeats_sparse", with_repeats(random_set(18, 64, 100), 100), 3));
    c = make("repeats_sparse_no_dedupe", with_repeats(random_set(18, 64, 100), 100), 3);
    c.T.dedupe = 0;
    r.push_back(c);
    c = make("repeats_dense", with_repeats(random_set(19, 600, 150), 150), 3);
    c.T.max_keys = 1024;
    r.push_back(c);
    c = make("repeats_dense_forced", with_repeats(random_set(20, 300, 150), 150), 3);
    c.T.dense = 2;
    c.T.dense_min_density = 3;
    r.push_back(c);
    r.push_back(make("exact_64_sparse", random_set(21, 100, 64), 3));
    c = make("dense_declined", random_set(22, 600, 64), 3); // (wanted, but 8/16 of the dimers do not cover the set)
    c.T.max_keys = 1024;
    r.push_back(c);
    c = make("unanchored_stride1", random_set(23, 600, 150), 3);
    c.T.max_keys = 1024;
    c.T.dense = 0;
    c.T.force_stride = 1;
    c.T.anchor = 0;
    r.push_back(c);
    c = make("too_many_passes", random_set(24, 4200, 150), 3);
    c.T.max_keys = 64;
    c.T.dense = 0;
    c.T.anchor = 0;
    r.push_back(c);
    c = make("shiftor_dense_forced", random_set(25, 300, 40), 0);
    c.algo = SPM_ALGO_SHIFTOR;
    c.T.dense = 2;
    r.push_back(c);
    {
        generator g(26);
        std::vector<needle> set;
        for (uint32_t m : {64u, 100u, 150u, 300u, 1000u, 2047u})
            set.push_back(random_needle(g, m));
        r.push_back(make("mixed_lengths", set, 3)); // (the stride follows the shortest seed)
    }
    {
        std::vector<needle> set = random_set(28, 8, 100);
        generator g(29);
        set[3] = random_needle(g, 2048); // (an entry holds a needle offset in 11 bits)
        r.push_back(make("needle_too_long", set, 3));
    }
    return r;
}

int run_cases()
{
    for (index_case c : all_cases()) {
        const flat_set S(c);
        for (int threads : {1, 4}) {
            c.T.threads = threads;
            seed_index X;
            const int rc = build_filter_index(S.nv, c.T, X);
            std::printf("%s threads=%d rc=%d passes=%zu stride=%u key_len=%u anchored=%d dense=%d variant=%u digest=%016llx\n",
                        c.name.c_str(), threads, rc, X.fidx.size(), X.filter_stride, X.filter_key_len, (int)X.filter_anchored,
                        (int)X.filter_dense, X.fidx.empty() ? 0u : X.fidx[0].hash_variant, (unsigned long long)digest(X));
        }
    }
    return 0;
}

int run_timing()
{
    index_case c = make("c4", random_set(100, 100000, 150), 3);
    const flat_set S(c);
    for (int dense : {1, 0}) {
        index_tuning T;
        T.threads = 16;
        T.dense = dense;
        seed_index X;
        const auto t0 = std::chrono::steady_clock::now();
        const int rc = build_filter_index(S.nv, T, X);
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        std::printf("%s rc=%d passes=%zu ms=%.3f\n", dense ? "c4_dense" : "c4_anchored", rc, X.fidx.size(), ms);
    }
    return 0;
}

} // namespace

int main(int argc, char **argv)
{
    return argc > 1 && std::strcmp(argv[1], "--time") == 0 ? run_timing() : run_cases();
}

// dense_census.cpp -- what the dense pass's tables look like for ONE needle set, without a device: the set is read from a
// file, built with build_filter_index (libspm_amd/csrc/index_build.hpp) under explicit tuning -- the environment is never
// read -- and one line per fact of the resulting seed_index / filter_index is printed.  tests/test_dense_states.py compares
// the lines with the rule written again in tests/dense_states.py.  Only what seed_index / filter_index already hold is
// printed; nothing is recomputed from the needles.
//
//   dense_census FILE DENSE THREADS
//
// FILE: four little-endian uint32 {n, m, algo, k}, then n * m symbol ranks (dna4), one needle after the other.
// DENSE: index_tuning::dense (1: when the plan wants it, 2: whenever the set admits it).  THREADS: 1 .. 16.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "index_build.hpp"

using namespace spm_hip;

namespace
{

bool read_exact(FILE *f, void *to, size_t bytes) { return bytes == 0 || fread(to, 1, bytes, f) == bytes; }

void print_list(const char *name, const std::vector<uint32_t> &v)
{
    std::printf("%s=", name);
    for (size_t i = 0; i < v.size(); ++i)
        std::printf(i ? ",%u" : "%u", v[i]);
    std::printf("\n");
}

} // namespace

int main(int argc, char **argv)
{
    if (argc != 4) {
        std::fprintf(stderr, "usage: dense_census FILE DENSE THREADS\n");
        return 2;
    }
    const int dense = std::atoi(argv[2]), threads = std::atoi(argv[3]);
    if (dense < 1 || dense > 2 || threads < 1 || threads > 16) {
        std::fprintf(stderr, "dense_census: DENSE is 1 or 2, THREADS 1 .. 16\n");
        return 2;
    }
    FILE *f = std::fopen(argv[1], "rb");
    uint32_t head[4] = {0, 0, 0, 0};
    if (!f || !read_exact(f, head, sizeof(head))) {
        std::fprintf(stderr, "dense_census: cannot read %s\n", argv[1]);
        return 2;
    }
    const uint32_t n = head[0], m = head[1], algo = head[2], k = head[3];
    if (n == 0 || n >= (1u << 21) || m == 0 || m > 2047 || k > 7) {
        std::fprintf(stderr, "dense_census: n, m or k out of range\n");
        return 2;
    }
    std::vector<uint8_t> ranks((size_t)n * m);
    const bool whole = read_exact(f, ranks.data(), ranks.size());
    std::fclose(f);
    if (!whole) {
        std::fprintf(stderr, "dense_census: %s is shorter than its header says\n", argv[1]);
        return 2;
    }
    for (uint8_t c : ranks)
        if (c > 3) {
            std::fprintf(stderr, "dense_census: a rank above 3\n");
            return 2;
        }
    std::vector<uint32_t> offsets(n + 1);
    for (uint32_t p = 0; p <= n; ++p)
        offsets[p] = p * m;
    const bool myers = (int)algo == SPM_ALGO_MYERS;
    std::vector<int32_t> ms(n, (int32_t)m), ks(n, myers ? (int32_t)k : 0);
    needle_view nv;
    nv.algo = (int)algo;
    nv.n = n;
    nv.sigma = 4;
    nv.ranks = ranks.data();
    nv.offsets = offsets.data();
    nv.m = ms.data();
    nv.k = ks.data();
    nv.max_k = myers ? k : 0;
    index_tuning T;
    T.dense = dense;
    T.threads = threads;
    seed_index X;
    const int rc = build_filter_index(nv, T, X);
    std::printf("rc=%d\npasses=%zu\ndense=%d\n", rc, X.fidx.size(), (int)X.filter_dense);
    if (rc != SPM_OK || X.fidx.size() != 1 || !X.filter_dense)
        return 0;
    const filter_index &F = X.fidx[0];
    const size_t n_buckets = F.h_buckets.size() / kDenseSlots;
    std::vector<uint32_t> accept_all, full;
    uint32_t largest = 0;
    for (size_t b = 0; b < n_buckets; ++b) {
        const uint16_t *bk = F.h_buckets.data() + b * kDenseSlots;
        uint32_t used = 0;
        for (uint32_t s = 0; s < kDenseSlots; ++s)
            used += bk[s] != 0 ? 1u : 0u;
        largest = used > largest ? used : largest;
        if (bk[kDenseSlots - 1] == kDenseAcceptAll)
            accept_all.push_back((uint32_t)b);
        else if (used == kDenseSlots)
            full.push_back((uint32_t)b);
    }
    uint64_t bits = 0;
    for (uint32_t w : F.h_image)
        bits += (uint64_t)__builtin_popcount(w);
    std::printf("hash_variant=%u\nkeys=%llu\nbucket_shift=%u\nbuckets=%zu\n", F.hash_variant, (unsigned long long)F.n_keys,
                F.bucket_shift, n_buckets);
    print_list("accept_all", accept_all);
    print_list("full", full);
    std::printf("largest_fill=%u\npresence_bits=%llu\npresence_table=%zu\n", largest, (unsigned long long)bits,
                F.h_image.size() * 32);
    std::printf("anchor_sixteenths=%d\nanchor_patterns=%u\n", __builtin_popcount(F.dimer_set), F.n_pat);
    for (uint32_t i = 0; i < F.n_pat; ++i)
        std::printf("pattern%u=%u/%u\n", i, F.pat_c[i], F.pat_cm[i]);
    return 0;
}

// jst_walk_core_cases.cpp -- what a (block, haplotype) cell of the pan-genome index owns and what its context spells
// (libspm_amd/csrc/jst_walk_core.hpp) on the host: the functions the build and fan-out kernels call, on host arrays.  A program
// of its own (plain g++, and g++ -fsanitize=address,undefined); every array has its exact size, so a read past one is what the
// sanitizer build is for.
//
// The model is the haplotype itself: the allele table applied by brute force, every symbol with the reference position it
// stems from (an alt symbol: its allele's position).  a_lo and hap_start are filled through the core (jst_alo_row,
// jst_cell_delta, a serial column prefix, jst_hap_start); then for every block j and haplotype h
//   * hap_start[j][h] = the model's count of symbols stemming from positions < jL; row n_blocks = the haplotype's length; the
//     owned ranges [hap_start[j], hap_start[j + 1]) partition the haplotype;
//   * lo, len and owned_from of jst_left_walk follow from hap_start and min(window - 1, hap_start);
//   * the runs of jst_run_cursor spell hap[h][lo, lo + len), every run inside the reference or the alt pool;
//   * equal signatures within a block mean equal bytes and equal owned_from;
//   * a cell that carries an allele beyond the 256 bits of the signature shares its signature with no other haplotype.
// The trees: one table of every edge (below) on references of 96 and 128 symbols, block lengths 16, 32, 128, windows 1, 2,
// 8, 40, 3 and 70 haplotypes; 300 SNPs on consecutive positions in one block of 512; a tree without alleles.
#include <algorithm>
#include <array>
#include <cstdio>
#include <cstring>
#include <map>
#include <vector>

#include "jst_walk_core.hpp"

using namespace spm_hip;

static int failures = 0, checks = 0;
#define EXPECT_TRUE(cond)                                                                                              \
    do {                                                                                                               \
        ++checks;                                                                                                      \
        if (!(cond)) {                                                                                                 \
            if (++failures <= 40)                                                                                      \
                std::printf("FAILED %s:%d: %s  [%s]\n", __FILE__, __LINE__, #cond, where);                             \
        }                                                                                                              \
    } while (0)

static char where[160] = "";

struct row
{
    uint64_t pos;
    uint32_t ref_len;
    std::vector<uint8_t> alt;
    std::vector<uint32_t> haps;
};

struct tree
{
    std::vector<uint8_t> ref;
    std::vector<row> rows; // sorted by pos, ref_len clamped to the reference (as spm_hip_jst_create does)
    uint32_t H = 0;
    // the table as the arrays of jst_dev
    std::vector<uint64_t> pos, aoff, cov;
    std::vector<uint32_t> rlen, alen;
    std::vector<uint8_t> pool;
    uint32_t cw = 0, max_rlen = 0;
    // the model: haplotype h and, per symbol, the reference position it stems from
    std::vector<std::vector<uint8_t>> hap;
    std::vector<std::vector<uint64_t>> stem;
};

static uint8_t ref_symbol(uint64_t i) { return (uint8_t)(((uint32_t)i * 2654435761u) >> 30); }

static std::vector<uint8_t> syms(const char *s)
{
    std::vector<uint8_t> v;
    for (; *s; ++s)
        v.push_back((uint8_t)(*s - '0'));
    return v;
}

static tree make_tree(uint64_t n_ref, uint32_t H, std::vector<row> rows)
{
    tree T;
    T.H = H;
    T.cw = (H + 63) / 64;
    for (uint64_t i = 0; i < n_ref; ++i)
        T.ref.push_back(ref_symbol(i));
    std::stable_sort(rows.begin(), rows.end(), [](const row &a, const row &b) { return a.pos < b.pos; });
    T.cov.assign(rows.size() * T.cw, 0);
    for (size_t i = 0; i < rows.size(); ++i) {
        row &r = rows[i];
        r.ref_len = (uint32_t)std::min<uint64_t>(r.ref_len, n_ref - r.pos);
        T.pos.push_back(r.pos);
        T.rlen.push_back(r.ref_len);
        T.alen.push_back((uint32_t)r.alt.size());
        T.aoff.push_back(T.pool.size());
        T.pool.insert(T.pool.end(), r.alt.begin(), r.alt.end());
        T.max_rlen = std::max(T.max_rlen, r.ref_len);
        for (uint32_t h : r.haps)
            T.cov[i * T.cw + (h >> 6)] |= 1ull << (h & 63);
    }
    T.rows = rows;
    T.hap.resize(H);
    T.stem.resize(H);
    for (uint32_t h = 0; h < H; ++h) {
        uint64_t r = 0;
        auto reference_to = [&](uint64_t end) {
            for (; r < end; ++r) {
                T.hap[h].push_back(T.ref[r]);
                T.stem[h].push_back(r);
            }
        };
        for (const row &a : rows) {
            if (std::find(a.haps.begin(), a.haps.end(), h) == a.haps.end())
                continue;
            std::snprintf(where, sizeof where, "table: allele at %llu on haplotype %u", (unsigned long long)a.pos, h);
            EXPECT_TRUE(a.pos >= r); // alleles that overlap on the reference share no haplotype
            reference_to(a.pos);
            for (uint8_t s : a.alt) {
                T.hap[h].push_back(s);
                T.stem[h].push_back(a.pos);
            }
            r = a.pos + a.ref_len;
        }
        reference_to(n_ref);
    }
    return T;
}

// Every edge on one table.  Lanes 0, 1, 2 are the haplotypes of a 3-haplotype tree; with more, haplotype h takes lane h % 3
// (so contexts are shared), and haplotypes 64 and 69 carry a SNP of their own (second coverage word).
static tree edge_tree(uint64_t N, uint32_t H)
{
    auto lane = [&](uint32_t k) {
        std::vector<uint32_t> v;
        for (uint32_t h = k; h < H; h += 3)
            v.push_back(h);
        return v;
    };
    auto both = [&](uint32_t k0, uint32_t k1) {
        std::vector<uint32_t> v = lane(k0), w = lane(k1);
        v.insert(v.end(), w.begin(), w.end());
        return v;
    };
    std::vector<row> rows = {
        {0, 0, syms("321"), lane(0)},           // an insertion at 0
        {0, 3, {}, lane(1)},                     // a deletion from 0
        {10, 1, syms("2"), lane(0)},
        {15, 34, {}, lane(2)},                   // [15, 49): spans the whole blocks [16, 32) and [32, 48) -- cells that own nothing
        {28, 8, {}, lane(1)},                    // [28, 36): overlaps the two below, on another haplotype; crosses 32
        {30, 4, {}, lane(0)},                    // [30, 34) ...
        {34, 1, syms("1"), lane(0)},             // ... and a SNP back to back with it
        {46, 0, syms("012301230123"), lane(1)},  // a left context that starts inside this alt (window 8 at block border 48)
        {60, 4, {}, lane(1)},                    // a deletion that ends on the border 64 ...
        {64, 0, syms("0123"), lane(1)},          // ... back to back with an insertion on the border ...
        {64, 1, syms("2"), lane(1)},             // ... and that with a SNP on the border
        {64, 6, {}, lane(2)},                    // a deletion that starts on the border ...
        {70, 0, syms("11"), lane(2)},            // ... back to back with an insertion
        {78, 5, {}, lane(2)},                    // [78, 83): crosses the border 80
        {N - 4, 14, {}, lane(2)},                // ref_len runs past n_ref; overlaps the SNP below, on another haplotype
        {N - 1, 1, syms("0"), both(0, 1)},       // a SNP at n_ref - 1 (lanes 0 and 1 share the contexts around it)
        {N, 0, syms("22013"), both(0, 1)},       // insertions at n_ref
        {N, 0, syms("3"), lane(2)},              // (behind a deletion that runs to n_ref)
    };
    if (H > 69) {
        rows.push_back({50, 1, syms("3"), {69}});
        rows.push_back({52, 1, syms("0"), {64}});
    }
    return make_tree(N, H, rows);
}

// 300 SNPs on consecutive positions of one block: more than the 256 bits of the signature.  Haplotypes 0 and 3 carry all of
// them, 1 all but one of the first 44 (the ones beyond the bit set), 2 the last 256 only.
static tree dense_tree()
{
    std::vector<row> rows;
    for (uint32_t s = 0; s < 300; ++s) {
        std::vector<uint32_t> hs = {0, 3};
        if (s != 3)
            hs.push_back(1);
        if (s >= 44)
            hs.push_back(2);
        rows.push_back({100 + s, 1, {(uint8_t)((ref_symbol(100 + s) + 1) & 3)}, hs});
    }
    return make_tree(640, 4, rows);
}

struct index_stats
{
    uint64_t contexts = 0, unique_contexts = 0, context_symbols = 0, haplotype_symbols = 0;
};

static index_stats check_tree(const tree &T, const char *name, uint64_t L, uint32_t window)
{
    const uint64_t n_ref = T.ref.size(), n_blocks = std::max<uint64_t>(1, (n_ref + L - 1) / L);
    const uint32_t H = T.H;
    std::vector<uint64_t> a_lo(n_blocks + 1), hap_start((n_blocks + 1) * H);
    jst_dev J{};
    J.ref = T.ref.data();
    J.n_ref = n_ref;
    J.pos = T.pos.data();
    J.rlen = T.rlen.data();
    J.alen = T.alen.data();
    J.aoff = T.aoff.data();
    J.alt = T.pool.data();
    J.cov = T.cov.data();
    J.n_alleles = T.pos.size();
    J.cw = T.cw;
    J.n_hap = H;
    J.max_rlen = T.max_rlen;
    J.window = window;
    J.n_groups = (H + kJstGroup - 1) / kJstGroup;
    J.L = L;
    J.n_blocks = n_blocks;
    J.jb = 0;
    J.je = n_blocks;
    J.a_lo = a_lo.data();
    J.hap_start = hap_start.data();
    for (uint64_t j = 0; j <= n_blocks; ++j)
        a_lo[j] = jst_alo_row(J.pos, J.n_alleles, L, n_blocks, j);
    for (uint32_t h = 0; h < H; ++h) { // the deltas' exclusive prefix down the column, row n_blocks the total; then the shift
        std::vector<int64_t> shift(n_blocks + 1, 0);
        for (uint64_t j = 0; j < n_blocks; ++j)
            shift[j + 1] = shift[j] + jst_cell_delta(J, j, h);
        for (uint64_t j = 0; j <= n_blocks; ++j)
            hap_start[j * H + h] = jst_hap_start(J, j, h, shift[j]);
    }
    index_stats S;
    uint64_t overflowing = 0, inside_alt = 0;
    for (uint64_t j = 0; j < n_blocks; ++j) {
        std::map<std::array<uint32_t, kJstSigWords>, uint32_t> first_of; // signature -> first haplotype that has it
        std::vector<std::vector<uint8_t>> bytes(H);
        std::vector<jst_walk> walks(H);
        std::vector<bool> beyond(H, false);
        for (uint32_t h = 0; h < H; ++h) {
            std::snprintf(where, sizeof where, "%s n_ref %llu L %llu window %u H %u: block %llu haplotype %u", name,
                          (unsigned long long)n_ref, (unsigned long long)L, window, H, (unsigned long long)j, h);
            const std::vector<uint8_t> &hap = T.hap[h];
            const uint64_t a = hap_start[j * H + h], b = hap_start[(j + 1) * H + h];
            const uint64_t want_a = (uint64_t)std::count_if(T.stem[h].begin(), T.stem[h].end(), [&](uint64_t s) { return s < j * L; });
            EXPECT_TRUE(a == want_a);
            EXPECT_TRUE(a <= b && b <= hap.size()); // with row 0 and row n_blocks below: a partition
            if (j == 0)
                EXPECT_TRUE(a == 0);
            if (j + 1 == n_blocks)
                EXPECT_TRUE(b == hap.size());
            jst_walk &W = walks[h];
            jst_left_walk(J, j, h, W);
            EXPECT_TRUE(W.empty == (a == b));
            if (a > b || b > hap.size() || W.empty)
                continue;
            const uint64_t left = std::min<uint64_t>(window - 1, a);
            EXPECT_TRUE(W.owned_from == left && W.lo == a - left && W.len == left + (b - a));
            jst_run_cursor C(W, h);
            const uint8_t *src = nullptr;
            uint64_t n = 0;
            bool inside = true;
            while (C.next(J, src, n) && bytes[h].size() <= hap.size()) {
                const bool in_ref = src >= J.ref && src + n <= J.ref + n_ref;
                const bool in_alt = src >= J.alt && src + n <= J.alt + T.pool.size();
                inside = inside && (n == 0 || in_ref || in_alt);
                if (n && (in_ref || in_alt))
                    bytes[h].insert(bytes[h].end(), src, src + n);
            }
            EXPECT_TRUE(inside);
            EXPECT_TRUE(bytes[h].size() == W.len && W.lo + W.len <= hap.size() &&
                        std::equal(bytes[h].begin(), bytes[h].end(), hap.begin() + (long)W.lo));
            ++S.contexts;
            inside_alt += W.kind == 1;
            S.haplotype_symbols += W.len - W.owned_from;
            std::array<uint32_t, kJstSigWords> sig;
            std::copy(W.sig, W.sig + kJstSigWords, sig.begin());
            for (uint64_t i = a_lo[j]; i < a_lo[j + 1]; ++i) // an allele of the cell beyond the bit set
                beyond[h] = beyond[h] || (jst_carried(J, i, h) && a_lo[j + 1] - 1 - i >= 32ull * kJstMaskWords);
            const auto it = first_of.find(sig);
            if (it == first_of.end()) {
                first_of[sig] = h;
                ++S.unique_contexts;
                S.context_symbols += W.len;
            } else {
                const uint32_t g = it->second;
                EXPECT_TRUE(bytes[g] == bytes[h] && walks[g].owned_from == W.owned_from);
                EXPECT_TRUE(!beyond[h] && !beyond[g]); // a context that is not shared
            }
            overflowing += beyond[h];
        }
    }
    std::snprintf(where, sizeof where, "%s L %llu window %u", name, (unsigned long long)L, window);
    uint64_t total = 0;
    for (uint32_t h = 0; h < H; ++h)
        total += T.hap[h].size();
    EXPECT_TRUE(S.haplotype_symbols == total);
    if (std::strcmp(name, "edge") == 0 && L == 16 && window == 8)
        EXPECT_TRUE(inside_alt > 0); // a left context that starts inside an alt (block border 48, the insertion at 46)
    if (std::strcmp(name, "dense") == 0)
        EXPECT_TRUE(overflowing == 3 && S.contexts == 8 && S.unique_contexts == 5); // haplotypes 0, 1, 3 in block 0, where
                                                                                    // nothing is shared; block 1 is one context
    return S;
}

int main()
{
    for (uint64_t N : {96, 128})
        for (uint32_t H : {3u, 70u}) {
            const tree T = edge_tree(N, H);
            for (uint64_t L : {16, 32, 128})
                for (uint32_t window : {1u, 2u, 8u, 40u}) {
                    const index_stats S = check_tree(T, "edge", L, window);
                    if (N == 96 && H == 3 && L == 16 && window == 8) {
                        // the tree tests/test_gpu_jst_edges.py indexes on the device: both sides assert these constants
                        std::printf("stats n_ref 96 H 3 L 16 window 8: contexts %llu unique_contexts %llu context_symbols %llu "
                                    "haplotype_symbols %llu\n", (unsigned long long)S.contexts, (unsigned long long)S.unique_contexts,
                                    (unsigned long long)S.context_symbols, (unsigned long long)S.haplotype_symbols);
                        std::snprintf(where, sizeof where, "the recorded statistics");
                        EXPECT_TRUE(S.contexts == 16 && S.unique_contexts == 15 && S.context_symbols == 315 && S.haplotype_symbols == 252);
                    }
                }
        }
    const tree D = dense_tree();
    for (uint32_t window : {8u, 40u})
        check_tree(D, "dense", 512, window);
    check_tree(make_tree(96, 3, {}), "bare", 32, 8);
    std::printf("%d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}

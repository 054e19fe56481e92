// bgzf_huffman_core_cases.cpp -- the dynamic Huffman code of a deflate block on the host (libspm_amd/csrc/bgzf_huffman_core.hpp):
// the length routine against an exhaustive search on small alphabets and against a textbook package-merge that keeps its item
// sets, on random and adversarial histograms; canonical codes; the run-length coder of the header; the padding; a token's code;
// and files written by the serial deflater with the flag for the Python side to take apart: bgzf_huffman_core_cases DIR writes
// DIR/<name>.<block_data>.raw and .bgzf.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../libspm_amd/csrc/bgzf_deflate_core.hpp"

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

static std::vector<uint8_t> lengths_of(const std::vector<uint32_t> &count, uint32_t limit)
{
    std::unique_ptr<huff_work> W(new huff_work);
    std::vector<uint8_t> len(count.size() + 1, 0xEE);
    huff_lengths(count.data(), (uint32_t)count.size(), limit, len.data(), *W, 0, 1, huff_serial{});
    EXPECT_TRUE(len.back() == 0xEE);
    len.pop_back();
    return len;
}
static uint64_t cost_of(const std::vector<uint32_t> &count, const std::vector<uint8_t> &len)
{
    uint64_t c = 0;
    for (size_t i = 0; i < count.size(); ++i)
        c += (uint64_t)count[i] * len[i];
    return c;
}
// sum of 2^(limit - len) over the coded symbols == 2^limit: Kraft sum exactly 1; a zero count has no code, no length is above
// the limit
static bool complete(const std::vector<uint32_t> &count, const std::vector<uint8_t> &len, uint32_t limit)
{
    uint64_t k = 0;
    for (size_t i = 0; i < count.size(); ++i) {
        if ((count[i] == 0) != (len[i] == 0) || len[i] > limit)
            return false;
        if (len[i])
            k += 1ull << (limit - len[i]);
    }
    return k == 1ull << limit;
}

// reference 1: every assignment of lengths 1 .. limit with Kraft sum <= 1
static uint64_t exhaustive(const std::vector<uint32_t> &w, uint32_t limit)
{
    const size_t n = w.size();
    std::vector<uint32_t> len(n, 1);
    uint64_t best = ~0ull;
    for (;;) {
        uint64_t k = 0, c = 0;
        for (size_t i = 0; i < n; ++i) {
            k += 1ull << (limit - len[i]);
            c += (uint64_t)w[i] * len[i];
        }
        if (k <= 1ull << limit && c < best)
            best = c;
        size_t i = 0;
        while (i < n && len[i] == limit)
            len[i++] = 1;
        if (i == n)
            break;
        ++len[i];
    }
    return best;
}

// reference 2: package-merge as the textbooks have it (Larmore and Hirschberg): every item carries the leaves it is made of
struct pm_item
{
    uint64_t w;
    std::vector<uint32_t> leaves;
};
static std::vector<uint8_t> package_merge(const std::vector<uint32_t> &count, uint32_t limit)
{
    std::vector<pm_item> leaves;
    for (uint32_t i = 0; i < count.size(); ++i)
        if (count[i])
            leaves.push_back({count[i], {i}});
    std::stable_sort(leaves.begin(), leaves.end(), [](const pm_item &a, const pm_item &b) { return a.w < b.w; });
    const size_t n = leaves.size();
    std::vector<pm_item> list = leaves;
    for (uint32_t l = 1; l < limit; ++l) {
        std::vector<pm_item> merged = leaves;
        for (size_t j = 0; j + 1 < list.size(); j += 2) {
            pm_item p{list[j].w + list[j + 1].w, list[j].leaves};
            p.leaves.insert(p.leaves.end(), list[j + 1].leaves.begin(), list[j + 1].leaves.end());
            merged.push_back(std::move(p));
        }
        std::stable_sort(merged.begin(), merged.end(), [](const pm_item &a, const pm_item &b) { return a.w < b.w; });
        list = std::move(merged);
    }
    std::vector<uint8_t> len(count.size(), 0);
    for (size_t j = 0; j < 2 * n - 2; ++j)
        for (uint32_t s : list[j].leaves)
            ++len[s];
    return len;
}

static uint64_t rng_state = 0;
static uint64_t rnd() { return mix64(++rng_state); }

static void check_histogram(const std::vector<uint32_t> &count, uint32_t limit)
{
    const std::vector<uint8_t> len = lengths_of(count, limit), want = package_merge(count, limit);
    EXPECT_TRUE(complete(count, len, limit));
    EXPECT_TRUE(complete(count, want, limit)); // (the reference itself)
    EXPECT_TRUE(cost_of(count, len) == cost_of(count, want));
    // the tie rule: a heavier symbol has no longer code, and of two equal ones the lower-numbered has no shorter code
    bool ordered = true;
    for (size_t i = 0; i < count.size(); ++i)
        for (size_t j = i + 1; j < count.size() && count.size() <= 64; ++j)
            if (count[i] && count[j])
                ordered = ordered && (count[i] < count[j] ? len[i] >= len[j] : count[i] > count[j] ? len[i] <= len[j] : len[i] >= len[j]);
    EXPECT_TRUE(ordered);
}

static void length_cases()
{
    // exhaustive search: 2 .. 7 symbols, limits 3 .. 5, small counts with many ties
    for (uint32_t n = 2; n <= 7; ++n)
        for (uint32_t limit = 3; limit <= 5; ++limit)
            for (int trial = 0; trial < 40; ++trial) {
                std::vector<uint32_t> w(n);
                for (uint32_t &x : w)
                    x = 1 + (uint32_t)(rnd() % (trial < 10 ? 3 : trial < 25 ? 12 : 1000));
                const std::vector<uint8_t> len = lengths_of(w, limit);
                EXPECT_TRUE(complete(w, len, limit));
                EXPECT_TRUE(cost_of(w, len) == exhaustive(w, limit));
            }
    // the textbook package-merge: limits 7 (up to 128 symbols) and 15
    for (uint32_t limit : {7u, 15u}) {
        const uint32_t most = limit == 7 ? 128 : 286;
        for (uint32_t n : {2u, 3u, 4u, 5u, 17u, 19u, 30u, 64u, 100u, 127u, 128u, 200u, 285u, 286u}) {
            if (n > most)
                continue;
            check_histogram(std::vector<uint32_t>(n, 1), limit);     // all equal (286 symbols of count 1 among them)
            check_histogram(std::vector<uint32_t>(n, 65280), limit);
            std::vector<uint32_t> w(n, 1);
            w[n / 2] = 65280;                                        // one dominant symbol
            check_histogram(w, limit);
            for (int trial = 0; trial < 6; ++trial) {                // random, with zero counts among them
                for (uint32_t &x : w)
                    x = trial == 0 ? (uint32_t)(rnd() % 65281) : trial == 1 ? 1 + (uint32_t)(rnd() % 4)
                        : rnd() % 3 == 0 ? 0 : (uint32_t)(rnd() >> (40 + rnd() % 20)) % 65281;
                w[0] = w[0] ? w[0] : 7;
                w[n - 1] = w[n - 1] ? w[n - 1] : 9;
                check_histogram(w, limit);
            }
            for (uint32_t &x : w)                                    // geometric: deeper than any limit allows
                x = 1u << ((&x - w.data()) % 16);
            check_histogram(w, limit);
        }
    }
    // Fibonacci counts 1, 1, 2, 3, ...: the unlimited code of 17 and more symbols is deeper than 15
    for (uint32_t n : {17u, 22u, 30u}) {
        std::vector<uint32_t> w(n, 1);
        for (uint32_t i = 2; i < n; ++i)
            w[i] = w[i - 1] + w[i - 2];
        check_histogram(w, 15);
        const std::vector<uint8_t> len = lengths_of(w, 15);
        EXPECT_TRUE(*std::max_element(len.begin(), len.end()) == 15);
        std::reverse(w.begin(), w.end());
        check_histogram(w, 15);
        // sparse inside the literal/length alphabet
        std::vector<uint32_t> wide(286, 0);
        for (uint32_t i = 0; i < n; ++i)
            wide[(i * 37) % 286] = w[i];
        check_histogram(wide, 15);
    }
    check_histogram({5, 9}, 15);                                     // two symbols
    check_histogram({1, 1}, 7);
    check_histogram({0, 0, 65280, 0, 1, 0}, 15);
    const std::vector<uint8_t> two = lengths_of({0, 3, 0, 0, 8}, 15);
    EXPECT_TRUE(two[1] == 1 && two[4] == 1 && two[0] == 0);
}

static void pad_cases()
{
    uint32_t a[6] = {0, 0, 0, 0, 0, 0};
    huff_pad(a, 6);
    EXPECT_TRUE(a[0] == 1 && a[1] == 1 && a[2] == 0);
    uint32_t b[6] = {0, 0, 0, 7, 0, 0};
    huff_pad(b, 6);
    EXPECT_TRUE(b[0] == 1 && b[1] == 0 && b[3] == 7);
    uint32_t c[6] = {9, 0, 0, 0, 0, 0};
    huff_pad(c, 6);
    EXPECT_TRUE(c[0] == 9 && c[1] == 1 && c[2] == 0);
    uint32_t d[6] = {0, 2, 0, 0, 3, 0};
    huff_pad(d, 6);
    EXPECT_TRUE(d[0] == 0 && d[1] == 2 && d[4] == 3);
}

// canonical codes: prefix-free, shorter codes first, within a length by symbol
static void code_cases()
{
    for (int trial = 0; trial < 30; ++trial) {
        std::vector<uint32_t> w(trial < 10 ? 19 : trial < 20 ? 30 : 286);
        for (uint32_t &x : w)
            x = rnd() % 4 == 0 ? 0 : 1 + (uint32_t)(rnd() % (1 + (rnd() % 60000)));
        w[0] = w[1] = 1;
        const uint32_t limit = w.size() == 19 ? 7 : 15;
        const std::vector<uint8_t> len = lengths_of(w, limit);
        std::vector<uint32_t> code(w.size());
        huff_codes(len.data(), (uint32_t)w.size(), code.data(), 0, 1);
        bool ok = true;
        for (size_t i = 0; i < w.size(); ++i) {
            ok = ok && (code[i] >> 16) == len[i] && (len[i] || code[i] == 0);
            for (size_t j = 0; j < w.size() && len[i]; ++j) {
                if (i == j || !len[j] || len[j] < len[i])
                    continue;
                // in stream order the first len[i] bits of j's code are its low bits
                ok = ok && ((code[j] & 0xffff) & ((1u << len[i]) - 1)) != (code[i] & 0xffff);
                const uint32_t ci = deflate_reverse(code[i] & 0xffff, len[i]), cj = deflate_reverse(code[j] & 0xffff, len[j]);
                if (len[j] == len[i])
                    ok = ok && (i < j) == (ci < cj);
                else
                    ok = ok && (ci << (len[j] - len[i])) < cj;
            }
        }
        EXPECT_TRUE(ok);
    }
    // RFC 1951 3.2.2's example: lengths (3, 3, 3, 3, 3, 2, 4, 4) -> 010 011 100 101 110 00 1110 1111
    const uint8_t len[8] = {3, 3, 3, 3, 3, 2, 4, 4};
    const uint32_t want[8] = {2, 3, 4, 5, 6, 0, 14, 15};
    uint32_t code[8];
    huff_codes(len, 8, code, 0, 1);
    for (int i = 0; i < 8; ++i)
        EXPECT_TRUE(deflate_reverse(code[i] & 0xffff, len[i]) == want[i] && (code[i] >> 16) == len[i]);
}

// the run-length coder: what it writes decodes back to the sequence, and is what the greedy rule says
static std::vector<uint32_t> unrun(const uint16_t *seq, uint32_t k)
{
    std::vector<uint32_t> out;
    for (uint32_t i = 0; i < k; ++i) {
        const uint32_t s = seq[i] & 0xff, x = seq[i] >> 8;
        if (s < 16)
            out.push_back(s);
        else if (s == 16)
            out.insert(out.end(), 3 + x, out.empty() ? 99u : out.back());
        else
            out.insert(out.end(), (s == 17 ? 3 : 11) + x, 0u);
    }
    return out;
}
static void run_cases()
{
    uint16_t seq[kHufSeq];
    for (uint32_t v : {0u, 5u})
        for (uint32_t run : {1u, 2u, 3u, 6u, 7u, 10u, 11u, 12u, 138u, 139u, 140u, 141u, 149u, 300u})
            for (uint32_t front : {0u, 1u})
                for (uint32_t behind : {0u, 2u}) {
                    std::vector<uint32_t> s(front, 9);
                    s.insert(s.end(), run, v);
                    s.insert(s.end(), behind, 3);
                    if (s.size() > kHufSeq)
                        continue;
                    const uint32_t k = huff_run_lengths([&](uint32_t i) { return s[i]; }, (uint32_t)s.size(), seq);
                    EXPECT_TRUE(k <= s.size() && unrun(seq, k) == s);
                    bool fits = true;
                    for (uint32_t i = 0; i < k; ++i) {
                        const uint32_t sym = seq[i] & 0xff, x = seq[i] >> 8;
                        fits = fits && sym <= 18 && x < (1u << huff_cl_extra_bits(sym));
                    }
                    EXPECT_TRUE(fits);
                    // the greedy rule, symbol by symbol, behind the front
                    std::vector<uint16_t> want;
                    if (v == 0) {
                        uint32_t r = run;
                        for (; r >= 3; r -= r < 138 ? r : 138)
                            want.push_back(r >= 11 ? (uint16_t)(18 | ((r < 138 ? r : 138) - 11) << 8) : (uint16_t)(17 | (r - 3) << 8));
                        want.insert(want.end(), r, (uint16_t)0);
                    } else {
                        uint32_t r = run - 1;
                        want.push_back((uint16_t)v);
                        for (; r >= 3; r -= r < 6 ? r : 6)
                            want.push_back((uint16_t)(16 | ((r < 6 ? r : 6) - 3) << 8));
                        want.insert(want.end(), r, (uint16_t)v);
                    }
                    EXPECT_TRUE(k == front + want.size() + behind && std::equal(want.begin(), want.end(), seq + front));
                }
    // a run across the literal/distance border, through the block build: literals 0, 1, 2 and the end of block once each,
    // distances 0 .. 3 once each: every length is 2, and the last literal/length entry and the four distance entries are ONE run
    std::unique_ptr<huff_work> W(new huff_work());
    huff_code K;
    for (uint32_t s : {0u, 1u, 2u, 256u, 286u, 287u, 288u, 289u})
        W->count[s] = 1;
    huff_block_build(*W, K, 0, 1, huff_serial{});
    EXPECT_TRUE(K.hlit == 0 && K.hdist == 3 && K.n_seq == 7);
    const uint16_t border[7] = {2, 2, 2, 18 | (138 - 11) << 8, 18 | (253 - 138 - 11) << 8, 2, 16 | (4 - 3) << 8};
    EXPECT_TRUE(std::equal(border, border + 7, K.seq));
    std::vector<uint32_t> all = unrun(K.seq, K.n_seq);
    EXPECT_TRUE(all.size() == 257 + 4 && all[256] == 2 && all[257] == 2 && all[260] == 2 && all[3] == 0);
    // the code-length code of that header: symbols 2 (x4), 16 and 18 (x2); HCLEN reaches symbol 2, the 16th of the permuted order
    EXPECT_TRUE(K.hclen == 16 - 4 && (K.cl[2] >> 16) == 1 && (K.cl[18] >> 16) == 2 && (K.cl[16] >> 16) == 2 && (K.cl[0] >> 16) == 0);
    EXPECT_TRUE(K.header_bits == 14 + 3 * 16 + 4 * 1 + 2 * (2 + 7) + (2 + 2));
    // random histograms: the header's sequence is the two length vectors back to back, the sizes add up
    for (int trial = 0; trial < 60; ++trial) {
        std::unique_ptr<huff_work> V(new huff_work());
        const uint32_t top_ll = 257 + (uint32_t)(rnd() % 30), top_dd = (uint32_t)(rnd() % 31);
        for (uint32_t i = 0; i < top_ll; ++i)
            V->count[i] = rnd() % (1 + trial % 5) ? 0 : 1 + (uint32_t)(rnd() % (trial % 2 ? 5 : 3000));
        for (uint32_t i = 0; i < top_dd; ++i)
            V->count[kHufLitLen + i] = rnd() % (1 + trial % 3) ? 0 : 1 + (uint32_t)(rnd() % (trial % 2 ? 3 : 500));
        V->count[kHufEob] = 1;
        huff_block_build(*V, K, 0, 1, huff_serial{});
        std::vector<uint32_t> want(V->len, V->len + K.hlit + 257);
        want.insert(want.end(), V->len + kHufLitLen, V->len + kHufLitLen + K.hdist + 1);
        EXPECT_TRUE(unrun(K.seq, K.n_seq) == want && want[K.hlit + 256] != 0 && want.back() != 0);
        uint64_t bits = 0;
        huff_put_header(K, [&](uint64_t, uint32_t n) { bits += n; });
        EXPECT_TRUE(bits == K.header_bits && K.hclen <= 15);
        uint32_t used_dd = 0;
        for (uint32_t i = 0; i < kHufDist; ++i)
            used_dd += V->len[kHufLitLen + i] != 0;
        EXPECT_TRUE(used_dd >= 2); // the padding: no decoder meets an empty or one-symbol distance code
        for (uint32_t len : {1u, 3u, 4u, 10u, 11u, 257u, 258u})
            for (uint32_t v : {1u, 2u, 5u, 300u, 32768u}) {
                deflate_code a, b;
                uint32_t ls, ds;
                huff_count_token(len, len == 1 ? v & 0xff : v, ls, ds);
                huff_token_code(K, len, len == 1 ? v & 0xff : v, a, b);
                EXPECT_TRUE(a.n + b.n == huff_token_bits(K, len, len == 1 ? v & 0xff : v) && a.n <= 20 && b.n <= 28);
                EXPECT_TRUE((a.bits >> a.n) == 0 && (b.bits >> b.n) == 0 && (len == 1) == (ds == kHufDist) && (len > 1 || ls == (v & 0xff)));
            }
    }
}

static std::vector<uint8_t> input(int kind, size_t n, uint64_t seed = 0)
{
    std::vector<uint8_t> v(n);
    for (size_t i = 0; i < n; ++i) {
        const uint64_t r = mix64(seed * 0x10001 + 0xD1A + i);
        switch (kind) {
        case 0: v[i] = (uint8_t)(r >> 17); break;                                     // random
        case 1: v[i] = 0xff; break;                                                   // one byte
        case 2: v[i] = (uint8_t)((r >> 20) % 40); break;                              // uniform over 40 values
        case 3: v[i] = (uint8_t)(2 + std::min<uint64_t>((r >> 8) % 40, (r >> 30) % 40)); break; // skewed, quality-like
        case 4: v[i] = (uint8_t)(mix64(i % 300 < 150 ? 7 : (i / 300) % 5 * 300 + i % 300) >> 11); break; // records: a run, a repeat
        default: v[i] = (i / 70000) % 3 == 0 ? (uint8_t)(r >> 17) : (i / 70000) % 3 == 1 ? (uint8_t)((r >> 20) % 5 + 150) : (uint8_t)"ab"[i & 1]; break;
        }
    }
    return v;
}

// one block both ways: the flag changes the coding, never the tokens; the choice is step 5's
static void block_cases()
{
    for (int kind = 0; kind < 6; ++kind)
        for (uint32_t d : {1u, 2u, 6u, 40u, 63u, 64u, 65u, 257u, 300u, 1000u, 4096u, 16385u, 65279u, 65280u}) {
            std::unique_ptr<uint8_t[]> heap(new uint8_t[d]); // the block ends where its allocation ends
            const std::vector<uint8_t> v = input(kind, d, d);
            memcpy(heap.get(), v.data(), d);
            std::vector<uint8_t> plain(d + kDefStored + 8, 0xAA), flagged(d + kDefStored + 8, 0xAA);
            deflate_counts c0, c1;
            const uint32_t m0 = deflate_block_serial(heap.get(), d, plain.data(), &c0), m1 = deflate_block_serial(heap.get(), d, flagged.data(), &c1, true);
            const uint32_t t0 = (plain[0] >> 1) & 3, t1 = (flagged[0] >> 1) & 3;
            EXPECT_TRUE(m1 <= m0 && m0 <= d + kDefStored && t0 != 2 && (plain[0] & 1) && (flagged[0] & 1));
            EXPECT_TRUE(t1 == 2 ? m1 < m0 : (t1 == t0 && m1 == m0 && memcmp(plain.data(), flagged.data(), m0) == 0));
            EXPECT_TRUE(c1.n_dynamic_blocks == (t1 == 2) && c0.n_dynamic_blocks == 0 && c1.n_stored_blocks == (t1 == 0));
            EXPECT_TRUE(t1 == 0 || (c1.n_matches + c1.n_literals > 0 && (t0 == 0 || (c1.n_matches == c0.n_matches && c1.n_literals == c0.n_literals))));
            bool clean = true;
            for (size_t i = m1; i < flagged.size(); ++i)
                clean = clean && flagged[i] == 0xAA; // nothing beyond the payload
            EXPECT_TRUE(clean);
            if (kind == 2 && d >= 1000)
                EXPECT_TRUE(t1 == 2 && m1 <= 3 * d / 4 + 400 - 26);
            if (kind == 1 && d >= 4096)
                EXPECT_TRUE(t1 == 2);
            if (kind == 0 && d >= 257)
                EXPECT_TRUE(t1 == 0);
            if (d <= 6)
                EXPECT_TRUE(t1 == 1);
        }
    EXPECT_TRUE(deflate_choose(10, 9, 20) == 2 && deflate_choose(10, 10, 20) == 1 && deflate_choose(30, 24, 20) == 2 && deflate_choose(25, 25, 20) == 0);
    EXPECT_TRUE(deflate_choose(24, 25, 20) == 1 && deflate_choose(25, 30, 20) == 0 && !huff_may_win(1, 0, 3) && huff_may_win(65280, 0, 65285));
}

static void write_file(const std::string &path, const std::vector<uint8_t> &v)
{
    FILE *f = std::fopen(path.c_str(), "wb");
    EXPECT_TRUE(f != nullptr);
    if (!f)
        return;
    EXPECT_TRUE(std::fwrite(v.data(), 1, v.size(), f) == v.size());
    std::fclose(f);
}

static void file_cases(const std::string &dir)
{
    const char *names[6] = {"random", "equal", "uniform40", "skewed", "records", "mixed"};
    for (int kind = 0; kind < 6; ++kind)
        for (uint32_t opt : {0u, 257u, 64u}) {
            const uint32_t D = bgzf_block_data(opt);
            const size_t n = opt == 0 ? (kind == 5 ? 3 * 70000 + 4321 : 2 * 65280 + 4321) : opt == 257 ? 5000 : 700;
            std::unique_ptr<uint8_t[]> heap(new uint8_t[n]);
            const std::vector<uint8_t> v = input(kind, n, 5);
            memcpy(heap.get(), v.data(), n);
            std::vector<uint8_t> out(bgzf_framed_size(n, D, true) + 8, 0xAA), again(out.size(), 0x55), plain(out.size());
            std::vector<uint64_t> offsets, plain_offsets;
            deflate_counts counts;
            const uint64_t len = bgzf_deflate_serial(heap.get(), n, D, true, out.data(), &offsets, &counts, true);
            const uint64_t plain_len = bgzf_deflate_serial(heap.get(), n, D, true, plain.data(), &plain_offsets);
            EXPECT_TRUE(len <= plain_len && plain_len <= bgzf_framed_size(n, D, true) && offsets.size() == bgzf_n_blocks(n, D) + 1 && offsets[0] == 0);
            EXPECT_TRUE(offsets.back() + kBgzfEof == len);
            for (size_t i = len; i < out.size(); ++i)
                EXPECT_TRUE(out[i] == 0xAA);
            EXPECT_TRUE(bgzf_deflate_serial(heap.get(), n, D, true, again.data(), nullptr, nullptr, true) == len && memcmp(out.data(), again.data(), len) == 0);
            uint64_t n_dynamic = 0;
            for (size_t b = 0; b + 1 < offsets.size(); ++b) {
                const uint32_t size = (uint32_t)(offsets[b + 1] - offsets[b]);
                EXPECT_TRUE(size <= plain_offsets[b + 1] - plain_offsets[b] && (out[offsets[b] + 16] | out[offsets[b] + 17] << 8) == (int)size - 1);
                n_dynamic += ((out[offsets[b] + 18] >> 1) & 3) == 2;
            }
            EXPECT_TRUE(n_dynamic == counts.n_dynamic_blocks);
            if (kind == 0 && opt != 64)
                EXPECT_TRUE(counts.n_stored_blocks == bgzf_n_blocks(n, D) && len == bgzf_framed_size(n, D, true));
            if ((kind == 2 || kind == 3) && opt != 64)
                EXPECT_TRUE(counts.n_dynamic_blocks == bgzf_n_blocks(n, D) && len < plain_len);
            out.resize(len);
            if (!dir.empty()) {
                const std::string stem = dir + "/" + names[kind] + "." + std::to_string(D);
                write_file(stem + ".raw", v);
                write_file(stem + ".bgzf", out);
            }
        }
}

int main(int argc, char **argv)
{
    length_cases();
    pad_cases();
    code_cases();
    run_cases();
    block_cases();
    file_cases(argc > 1 ? argv[1] : "");
    std::printf("%d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}

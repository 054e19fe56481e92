// bgzf_deflate_core_cases.cpp -- the deflated container on the host (libspm_amd/csrc/bgzf_deflate_core.hpp): the fixed-Huffman
// code of a token against tables copied out of RFC 1951, the token rule's invariants (tokens tile every chunk, a match's source
// lies in the block and within 32768, replaying the tokens gives the data back, their bits add up to the payload's length),
// blocks that end where a heap allocation ends, and files for the Python side to inflate: bgzf_deflate_core_cases DIR writes
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

// a code as RFC 1951 prints it: the first bit of the stream on the left
static std::string printed(uint64_t bits, uint32_t n)
{
    std::string s;
    for (uint32_t i = 0; i < n; ++i)
        s += (bits >> i) & 1 ? '1' : '0';
    return s;
}

// RFC 1951, 3.2.5
static const uint32_t kLenBase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
static const uint32_t kLenExtra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
static const uint32_t kDistBase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
static const uint32_t kDistExtra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};

static void table_cases()
{
    uint32_t n = 0;
    EXPECT_TRUE(printed(deflate_token_code(1, 0).bits, deflate_token_code(1, 0).n) == "00110000");
    EXPECT_TRUE(printed(deflate_token_code(1, 143).bits, 8) == "10111111" && deflate_token_code(1, 143).n == 8);
    EXPECT_TRUE(printed(deflate_token_code(1, 144).bits, deflate_token_code(1, 144).n) == "110010000");
    EXPECT_TRUE(printed(deflate_token_code(1, 255).bits, deflate_token_code(1, 255).n) == "111111111");
    EXPECT_TRUE(deflate_litlen_code(256, n) == 0 && n == 7 && kDefEobBits == 7);
    EXPECT_TRUE(deflate_litlen_code(279, n) == 0x17 && n == 7);
    EXPECT_TRUE(deflate_litlen_code(280, n) == 0xC0 && n == 8); // 11000000
    EXPECT_TRUE(deflate_litlen_code(287, n) == 0xC7 && n == 8);
    uint32_t sym, e, x;
    deflate_len_symbol(3, sym, e, x);
    EXPECT_TRUE(sym == 257 && e == 0);
    deflate_len_symbol(257, sym, e, x);
    EXPECT_TRUE(sym == 284 && e == 5 && x == 30);
    deflate_len_symbol(258, sym, e, x);
    EXPECT_TRUE(sym == 285 && e == 0);
    deflate_dist_symbol(1, sym, e, x);
    EXPECT_TRUE(sym == 0 && e == 0);
    deflate_dist_symbol(32768, sym, e, x);
    EXPECT_TRUE(sym == 29 && e == 13 && x == 8191);
    // every length and every distance against the tables
    for (uint32_t len = 3; len <= 258; ++len) {
        uint32_t k = 28;
        while (kLenBase[k] > len)
            --k;
        if (len == 258)
            k = 28;
        else if (k == 28)
            k = 27;
        deflate_len_symbol(len, sym, e, x);
        EXPECT_TRUE(sym == 257 + k && e == kLenExtra[k] && x == len - kLenBase[k]);
    }
    for (uint32_t dist = 1; dist <= 32768; ++dist) {
        uint32_t k = 29;
        while (kDistBase[k] > dist)
            --k;
        deflate_dist_symbol(dist, sym, e, x);
        EXPECT_TRUE(sym == k && e == kDistExtra[k] && x == dist - kDistBase[k]);
    }
    // a token's size is its code's length; the code is Huffman code, extra bits, 5-bit distance code, extra bits
    for (uint32_t v = 0; v < 256; ++v)
        EXPECT_TRUE(deflate_token_bits(1, v) == deflate_token_code(1, v).n && deflate_token_code(1, v).n == (v < 144 ? 8u : 9u));
    for (uint32_t len = 3; len <= 258; ++len)
        for (uint32_t dist : {1u, 2u, 4u, 5u, 6u, 7u, 24u, 25u, 255u, 256u, 257u, 4096u, 4097u, 24576u, 24577u, 32767u, 32768u}) {
            const deflate_code c = deflate_token_code(len, dist);
            EXPECT_TRUE(c.n == deflate_token_bits(len, dist) && c.n <= 31 && (c.bits >> c.n) == 0);
            uint32_t ls, le, lx, ds, de, dx, hn;
            deflate_len_symbol(len, ls, le, lx);
            deflate_dist_symbol(dist, ds, de, dx);
            const uint32_t h = deflate_litlen_code(ls, hn);
            std::string want;
            for (uint32_t i = hn; i-- > 0;)
                want += (h >> i) & 1 ? '1' : '0';
            want += printed(lx, le);
            for (uint32_t i = 5; i-- > 0;)
                want += (ds >> i) & 1 ? '1' : '0';
            want += printed(dx, de);
            EXPECT_TRUE(printed(c.bits, c.n) == want);
        }
    // length 3 at distance 1: 0000001 00000;  length 258 at distance 32768: 11000101 11101 1111111111111
    EXPECT_TRUE(printed(deflate_token_code(3, 1).bits, 12) == "000000100000" && deflate_token_bits(3, 1) == 12);
    EXPECT_TRUE(printed(deflate_token_code(258, 32768).bits, 26) == "11000101111011111111111111");
    EXPECT_TRUE(deflate_chunk(1) == 64 && deflate_chunk(16384) == 64 && deflate_chunk(16385) == 65 && deflate_chunk(65280) == 255);
}

static std::vector<uint8_t> input(int kind, size_t n, uint64_t seed = 0)
{
    std::vector<uint8_t> v(n);
    for (size_t i = 0; i < n; ++i) {
        const uint64_t r = mix64(seed * 0x10001 + 0xDEF1 + i);
        switch (kind) {
        case 0: v[i] = (uint8_t)(r >> 17); break;                                     // random
        case 1: v[i] = 0xff; break;                                                   // one byte
        case 2: v[i] = (uint8_t)(mix64(i % 3) >> 9); break;                            // period 3
        case 3: v[i] = (uint8_t)(mix64(i % 257) >> 9); break;                          // period 257
        case 4: v[i] = (uint8_t)(mix64(i % 300 < 150 ? 7 : (i / 300) % 5 * 300 + i % 300) >> 11); break; // records: a run, a repeat
        default: v[i] = (i / 1000) & 1 ? (uint8_t)(r >> 17) : (uint8_t)((r >> 20) % 3 + 150); break;      // stretches of both
        }
    }
    return v;
}

// the invariants of the token rule over one block at p (exactly d bytes may be read)
static void block_cases(const uint8_t *p, uint32_t d)
{
    std::vector<deflate_token> tokens;
    const uint64_t bits = deflate_parse_serial(p, d, tokens);
    const uint32_t c = deflate_chunk(d);
    std::vector<uint8_t> replay(d);
    uint32_t at = 0;
    uint64_t sum = 0;
    bool ok = true;
    for (const deflate_token &k : tokens) {
        ok = ok && k.at == at && k.len >= 1 && at + k.len <= d;
        ok = ok && at / c == (at + k.len - 1) / c; // inside one chunk
        if (!ok)
            break;
        if (k.len == 1) {
            ok = ok && k.v == p[at];
            replay[at] = (uint8_t)k.v;
        } else {
            ok = ok && k.len >= kDefMinRun && k.len <= kDefMaxMatch && k.v >= 1 && k.v <= kDefMaxDist && k.v <= at;
            ok = ok && (k.len >= kDefMinMatch || k.v == 1);
            for (uint32_t i = 0; ok && i < k.len; ++i)
                replay[at + i] = replay[at + i - k.v];
        }
        sum += deflate_token_code(k.len, k.v).n;
        at += k.len;
    }
    EXPECT_TRUE(ok && at == d && sum == bits && memcmp(replay.data(), p, d) == 0);
    std::vector<uint8_t> out(d + kDefStored + 8, 0xAA);
    deflate_counts counts;
    const uint32_t m = deflate_block_serial(p, d, out.data(), &counts);
    const uint32_t fixed = (uint32_t)((3 + bits + 7 + 7) / 8);
    EXPECT_TRUE(m == (fixed < d + 5 ? fixed : d + 5) && m <= d + 5);
    EXPECT_TRUE((out[0] & 7) == (fixed < d + 5 ? 3 : 1));
    EXPECT_TRUE(counts.n_stored_blocks == (fixed < d + 5 ? 0u : 1u));
    EXPECT_TRUE(fixed >= d + 5 || counts.n_matches + counts.n_literals == tokens.size());
    for (size_t i = m; i < out.size(); ++i)
        ok = ok && out[i] == 0xAA; // nothing beyond the payload
    EXPECT_TRUE(ok);
}

static void rule_cases()
{
    for (int kind = 0; kind < 6; ++kind)
        for (uint32_t d : {1u, 2u, 3u, 4u, 5u, 63u, 64u, 65u, 255u, 256u, 257u, 258u, 259u, 260u, 511u, 512u, 515u, 4096u, 16384u, 16385u, 40000u, 65279u, 65280u}) {
            // the block ends where its allocation ends: a read past the source ends a sanitized run
            std::unique_ptr<uint8_t[]> heap(new uint8_t[d]);
            const std::vector<uint8_t> v = input(kind, d, d);
            memcpy(heap.get(), v.data(), d);
            block_cases(heap.get(), d);
        }
    // the far candidate is the LARGEST earlier position of the hash, from earlier segments only
    std::vector<uint8_t> v = input(0, 3000, 77);
    for (uint32_t at : {100u, 700u, 1500u})
        memcpy(v.data() + at, "abcdefgh", 8);
    memcpy(v.data() + 2000, "abcdefgh", 8);
    memcpy(v.data() + 2010, "abcdefgh", 8); // (2000 is in the same segment as 2010: not a candidate)
    std::vector<uint16_t> cand;
    deflate_candidates_serial(v.data(), 3000, cand);
    EXPECT_TRUE(cand[100] == 0 && cand[700] == 101 && cand[1500] == 701 && cand[2000] == 1501 && cand[2010] == 1501);
    EXPECT_TRUE(cand[2997] == 0 && cand[2998] == 0 && cand[2999] == 0); // fewer than four bytes behind them
    // exactly 32768 back is a match, 32769 is not
    for (uint32_t dist : {32768u, 32769u}) {
        std::vector<uint8_t> w = input(0, dist + 600, dist);
        memcpy(w.data() + dist, w.data(), 300);
        std::vector<deflate_token> tokens;
        deflate_parse_serial(w.data(), (uint32_t)w.size(), tokens);
        uint32_t far = 0;
        for (const deflate_token &k : tokens)
            far = std::max(far, k.len > 1 ? k.v : 0u);
        EXPECT_TRUE(far == (dist == 32768 ? 32768u : 0u) || (dist == 32769 && far < 32768));
        block_cases(w.data(), (uint32_t)w.size());
    }
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
    const char *names[6] = {"random", "equal", "period3", "period257", "records", "mixed"};
    for (int kind = 0; kind < 6; ++kind)
        for (uint32_t opt : {0u, 257u, 64u}) {
            const uint32_t D = bgzf_block_data(opt);
            const size_t n = opt == 0 ? 2 * 65280 + 4321 : opt == 257 ? 5000 : 700;
            std::unique_ptr<uint8_t[]> heap(new uint8_t[n]);
            const std::vector<uint8_t> v = input(kind, n, 5);
            memcpy(heap.get(), v.data(), n);
            std::vector<uint8_t> out(bgzf_framed_size(n, D, true) + 8, 0xAA), again(out.size(), 0x55);
            std::vector<uint64_t> offsets;
            deflate_counts counts;
            const uint64_t len = bgzf_deflate_serial(heap.get(), n, D, true, out.data(), &offsets, &counts);
            EXPECT_TRUE(len <= bgzf_framed_size(n, D, true) && offsets.size() == bgzf_n_blocks(n, D) + 1 && offsets[0] == 0);
            EXPECT_TRUE(offsets.back() + kBgzfEof == len);
            for (size_t i = len; i < out.size(); ++i)
                EXPECT_TRUE(out[i] == 0xAA);
            EXPECT_TRUE(bgzf_deflate_serial(heap.get(), n, D, true, again.data()) == len && memcmp(out.data(), again.data(), len) == 0);
            for (size_t b = 0; b + 1 < offsets.size(); ++b) {
                const uint32_t size = (uint32_t)(offsets[b + 1] - offsets[b]);
                EXPECT_TRUE(size <= bgzf_block_len(n, D, b) + kBgzfFrame && (out[offsets[b] + 16] | out[offsets[b] + 17] << 8) == (int)size - 1);
            }
            if (kind == 0 && opt != 64)
                EXPECT_TRUE(counts.n_stored_blocks == bgzf_n_blocks(n, D) && len == bgzf_framed_size(n, D, true));
            if (kind == 1 || (kind == 4 && opt != 64)) // (64 bytes without a repeat in them do not shrink)
                EXPECT_TRUE(counts.n_stored_blocks == 0 && counts.n_matches > 0 && len < bgzf_framed_size(n, D, true));
            out.resize(len);
            if (!dir.empty()) {
                const std::string stem = dir + "/" + names[kind] + "." + std::to_string(D);
                write_file(stem + ".raw", v);
                write_file(stem + ".bgzf", out);
            }
        }
    std::vector<uint8_t> eof(kBgzfEof);
    EXPECT_TRUE(bgzf_deflate_serial(nullptr, 0, 65280, true, eof.data()) == kBgzfEof && eof[0] == 0x1f && eof[16] == 0x1b);
    EXPECT_TRUE(bgzf_deflate_serial(nullptr, 0, 65280, false, eof.data()) == 0);
}

int main(int argc, char **argv)
{
    table_cases();
    rule_cases();
    file_cases(argc > 1 ? argv[1] : "");
    std::printf("%d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}

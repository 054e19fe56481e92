// bam_markdup_core_cases.cpp -- the rule of duplicate marking on the host (libspm_amd/csrc/bam_markdup_core.hpp): the 5' end of
// a record for every CIGAR op and both strands, item by item as the wave walks it and against bam_rec_end; the score of a run
// of quality bytes by dwords on the borders of the address against the byte walk, at every alignment of the buffer, of the
// record and of the run, with the stream's last dword short; the keys and what they order; the worked cases of spm_hip.h; what
// the serial builder refuses; and on a few thousand random small record sets the serial builder against a brute-force
// all-pairs comparison and against the device's scheme -- two stable sorts and "my key is my left neighbour's" -- replayed
// with std::stable_sort over the same key functions.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <random>
#include <vector>

#include "../../libspm_amd/csrc/bam_markdup_core.hpp"

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

static uint32_t W(uint32_t n, uint32_t op) { return n << 4 | op; }
static uint32_t EQ(uint32_t n) { return W(n, 7); }

// ---- a synthetic record stream: 36 fixed bytes, a name with its NUL, the CIGAR words, a SEQ, the qualities ----
struct rec
{
    uint32_t read = 0, flag = 0;
    int32_t ref_id = 0, pos = 0;
    std::vector<uint32_t> cigar;
    std::vector<uint8_t> qual; // l_seq values
    uint32_t name_len = 1;
};
struct stream
{
    std::vector<uint8_t> bytes;
    std::vector<spm_sam_line> lines;
    void put32(uint32_t v)
    {
        for (int i = 0; i < 4; ++i)
            bytes.push_back((uint8_t)(v >> (8 * i)));
    }
    void add(const rec &r)
    {
        const uint32_t l_seq = (uint32_t)r.qual.size();
        const uint32_t len = 36 + r.name_len + 1 + 4 * (uint32_t)r.cigar.size() + (l_seq + 1) / 2 + l_seq;
        spm_sam_line L{};
        L.offset = bytes.size();
        L.len = len;
        L.read = r.read;
        L.flag = (uint16_t)r.flag;
        lines.push_back(L);
        put32(len - 4);
        put32((uint32_t)r.ref_id);
        put32((uint32_t)r.pos);
        put32((r.name_len + 1) | 4680u << 16);
        put32((uint32_t)r.cigar.size() | r.flag << 16);
        put32(l_seq);
        put32(~0u);
        put32(~0u);
        put32(0);
        bytes.insert(bytes.end(), r.name_len, (uint8_t)'r');
        bytes.push_back(0);
        for (uint32_t w : r.cigar)
            put32(w);
        bytes.insert(bytes.end(), (l_seq + 1) / 2, 0x11);
        bytes.insert(bytes.end(), r.qual.begin(), r.qual.end());
    }
    bool mark(uint64_t ref_len, uint32_t min_qual, std::vector<uint8_t> &dup, md_counts &C) const
    {
        dup.assign(lines.size(), 7);
        return markdup_serial(bytes.data(), bytes.size(), lines.data(), lines.size(), ref_len, min_qual, dup.data(), C);
    }
};

// ---- the 5' end ----
static void end_cases()
{
    const std::vector<std::vector<uint32_t>> cigars = {
        {EQ(40)}, {W(10, 0), W(3, 1), W(5, 2), W(7, 3), W(2, 7), W(9, 8), W(4, 6)}, {}, {W(5, 1)}, {W(1, 0)},
        {W(268435455, 2)}, {EQ(3), W(1, 1), EQ(3), W(1, 2), EQ(3)}};
    std::vector<uint32_t> many; // more items than a wave has lanes
    for (uint32_t i = 0; i < 150; ++i)
        many.push_back(W(1 + i % 5, i % 3 == 1 ? 1 : i % 3 == 2 ? 2 : 7));
    auto all = cigars;
    all.push_back(many);
    for (const auto &cg : all)
        for (uint32_t flag : {0u, 16u})
            for (uint32_t name_len : {1u, 2u, 3u, 4u}) {
                stream S;
                rec r;
                r.flag = flag;
                r.pos = 1000;
                r.cigar = cg;
                r.name_len = name_len;
                r.qual.assign(5, 30);
                S.add(r);
                md_rec M;
                EXPECT_TRUE(md_rec_read(S.bytes.data(), S.bytes.size(), 0, S.lines[0].len, M));
                uint64_t span = 0, want_span = 0;
                bool clipped = false;
                md_cigar_walk(S.bytes.data(), M.R, span, clipped);
                for (uint32_t w : cg)
                    want_span += ((w & 15) == 0 || (w & 15) == 2 || (w & 15) == 3 || (w & 15) == 7 || (w & 15) == 8) ? w >> 4 : 0;
                EXPECT_TRUE(span == want_span && !clipped);
                // as the wave walks it: lane l takes the items l, l + 64, ...; the partial sums add up
                uint64_t lanes = 0;
                bool any = false;
                for (uint32_t lane = 0; lane < 64; ++lane) {
                    uint64_t part = 0;
                    bool c = false;
                    for (uint32_t k = lane; k < M.R.n_cigar_op; k += 64)
                        md_cigar_item(bam_u32(S.bytes.data() + 36 + name_len + 1 + 4 * k), part, c);
                    lanes += part;
                    any = any || c;
                }
                EXPECT_TRUE(lanes == span && !any);
                uint32_t u = 9, s = 9;
                const uint64_t end = bam_rec_end(S.bytes.data(), M.R);
                EXPECT_TRUE(end == 1000 + std::max<uint64_t>(span, 1));
                EXPECT_TRUE(md_end_of(M.R, span, clipped, end, u, s)); // end == ref_len
                EXPECT_TRUE(s == (flag >> 4) && u == (s ? end - 1 : 1000));
                EXPECT_TRUE(!md_end_of(M.R, span, clipped, end - 1, u, s));
                EXPECT_TRUE(!md_end_of(M.R, span, true, end, u, s));
                bam_rec R2 = M.R;
                R2.ref_id = 1;
                EXPECT_TRUE(!md_end_of(R2, span, clipped, end, u, s));
                R2 = M.R;
                R2.ref_id = -1;
                EXPECT_TRUE(!md_end_of(R2, span, clipped, end, u, s));
                R2 = M.R;
                R2.pos = -1;
                EXPECT_TRUE(!md_end_of(R2, span, clipped, 1 << 20, u, s));
            }
    for (uint32_t op : {4u, 5u}) { // S and H, in front and behind
        uint64_t span = 0;
        bool clipped = false;
        md_cigar_item(W(5, op), span, clipped);
        EXPECT_TRUE(span == 0 && clipped);
        md_cigar_item(EQ(7), span, clipped);
        EXPECT_TRUE(span == 7 && clipped);
    }
    EXPECT_TRUE(md_is_primary(0) && md_is_primary(0x400 | 0x10 | 0x1 | 0x4) && !md_is_primary(0x100) && !md_is_primary(0x800) && !md_is_primary(0x900));
}

// ---- the score: dwords on the borders of the ADDRESS, as md_ends_kernel loads them ----
static uint64_t score_by_dwords(const uint8_t *stream, uint64_t n_bytes, uint64_t q0, uint64_t q1, uint32_t min_qual)
{
    const uint64_t a0 = q0 - ((reinterpret_cast<uintptr_t>(stream) + q0) & 3u);
    uint64_t sum = 0;
    for (uint64_t at = a0; at < q1; at += 4) {
        uint32_t w = 0;
        EXPECT_TRUE((reinterpret_cast<uintptr_t>(stream + at) & 3u) == 0);
        for (uint32_t j = 0; j < 4 && at + j < n_bytes; ++j) // (the stream's last dword may be short)
            w |= (uint32_t)stream[at + j] << (8 * j);
        sum += md_score_dword(w, at, q0, q1, min_qual);
    }
    return sum;
}

static void score_cases()
{
    std::mt19937 rng(4242);
    alignas(8) static uint8_t buf[4096];
    for (uint32_t shift = 0; shift < 4; ++shift)          // the buffer's own alignment
        for (uint32_t name_len = 1; name_len <= 4; ++name_len)  // moves qual inside the record
            for (uint32_t lead = 0; lead < 2; ++lead)     // a record in front moves the record
                for (uint32_t l_seq : {0u, 1u, 2u, 3u, 4u, 5u, 7u, 8u, 30u, 63u, 64u, 65u, 150u, 255u, 256u, 257u, 300u}) {
                    stream S;
                    rec r;
                    if (lead) {
                        r.qual.assign(1 + l_seq % 7, 93);
                        r.cigar = {EQ(1)};
                        S.add(r);
                    }
                    r.read = lead;
                    r.name_len = name_len;
                    r.cigar = {EQ(std::max(l_seq, 1u))};
                    r.qual.resize(l_seq);
                    for (auto &q : r.qual)
                        q = (uint8_t)(rng() % 4 == 0 ? rng() % 256 : rng() % 94); // values beyond 93, and ff, among them
                    S.add(r);
                    uint8_t *p = buf + shift;
                    std::memset(buf, 0x5d, sizeof(buf)); // 93 around the stream: a byte outside the run must not count
                    std::memcpy(p, S.bytes.data(), S.bytes.size());
                    const spm_sam_line &L = S.lines[lead];
                    md_rec M;
                    EXPECT_TRUE(md_rec_read(p, S.bytes.size(), L.offset, L.len, M));
                    EXPECT_TRUE(M.l_seq == l_seq && L.offset + M.qual_at + l_seq == S.bytes.size());
                    for (uint32_t min_qual : {1u, 15u, 93u}) {
                        uint64_t want = 0;
                        for (uint8_t q : r.qual)
                            want += (q >= min_qual && q <= 93) ? q : 0;
                        const uint64_t q0 = L.offset + M.qual_at;
                        EXPECT_TRUE(md_score_bytes(p + q0, l_seq, min_qual) == want);
                        EXPECT_TRUE(score_by_dwords(p, S.bytes.size(), q0, q0 + l_seq, min_qual) == want);
                    }
                }
    EXPECT_TRUE(md_score_clamp(0) == 0 && md_score_clamp(kMdMaxScore - 1) == kMdMaxScore - 1 && md_score_clamp(kMdMaxScore) == kMdMaxScore &&
                md_score_clamp(1ull << 40) == kMdMaxScore);
    EXPECT_TRUE(md_min_qual(0) == 15 && md_min_qual(1) == 1 && md_min_qual(93) == 93);
    EXPECT_TRUE(md_qual_value(255, 1) == 0 && md_qual_value(94, 1) == 0 && md_qual_value(93, 93) == 93 && md_qual_value(14, 15) == 0);
}

// ---- the keys ----
static void key_cases()
{
    for (uint64_t ref_len : {1ull, 2ull, 1000ull, (1ull << 29), (1ull << 30) - 1}) {
        const uint32_t pb = bam_pos_bits(ref_len);
        EXPECT_TRUE((ref_len >> pb) == 0 && md_key_bits(true, pb) <= 64 && md_key_bits(true, pb) == 2 * pb + 3 && md_key_bits(false, pb) == pb + 3);
        const uint32_t top = (uint32_t)(ref_len - 1);
        // info: reads 0,1 a pair at (top, -) / (0, +); read 2 a fragment at (top, -); read 3 not placed; reads 4, 5: 5 lacks 0x1
        const unsigned long long info[6] = {md_info_pack(top, 1, true, 7), md_info_pack(0, 0, true, kMdMaxScore), md_info_pack(top, 1, false, 9), 0,
                                            md_info_pack(5 % ref_len, 0, true, 1), md_info_pack(5 % ref_len, 0, false, 2)};
        EXPECT_TRUE(md_is_pair_end(info, 6, 0) && md_is_pair_end(info, 6, 1) && !md_is_pair_end(info, 6, 2) && !md_is_pair_end(info, 6, 3) &&
                    !md_is_pair_end(info, 6, 4) && !md_is_pair_end(info, 6, 5) && !md_is_pair_end(info, 3, 2));
        EXPECT_TRUE(md_score(info[1]) == kMdMaxScore && md_score(info[0]) == 7 && md_end_code(info[0]) == ((uint64_t)top << 1 | 1));
        const uint64_t k0 = md_item_key(true, info, 6, 0, pb), k1 = md_item_key(true, info, 6, 1, pb), k2 = md_item_key(true, info, 6, 2, pb);
        EXPECT_TRUE(md_key_valid(true, k0, pb) && !md_key_valid(true, k1, pb) && !md_key_valid(true, k2, pb));
        EXPECT_TRUE(k0 == ((uint64_t)0 << (pb + 1) | ((uint64_t)top << 1 | 1)) && k0 < md_key_none(true, pb) && k1 == md_key_none(true, pb));
        EXPECT_TRUE(md_item_key(true, info, 5, 2, pb) == md_key_none(true, pb)); // an odd count: the last read has no mate
        EXPECT_TRUE(md_item_inv_score(true, info, 6, 0) == 2ull * kMdMaxScore - 7 - kMdMaxScore && md_item_inv_score(true, info, 5, 2) == 0);
        const uint64_t e0 = md_item_key(false, info, 6, 0, pb), e2 = md_item_key(false, info, 6, 2, pb), e3 = md_item_key(false, info, 6, 3, pb);
        EXPECT_TRUE(e0 + 1 == e2 && (e0 & 1) == 0 && md_key_valid(false, e2, pb) && !md_key_valid(false, e3, pb) && e2 < e3);
        EXPECT_TRUE(md_item_is_dup(false, e2, e0, pb) && !md_item_is_dup(false, e0, e0, pb) && !md_item_is_dup(false, e3, e3, pb));
        EXPECT_TRUE(md_item_is_dup(true, k0, k0, pb) && !md_item_is_dup(true, k1, k1, pb) && !md_item_is_dup(true, k0, k0 ^ 1, pb));
        EXPECT_TRUE(md_item_inv_score(false, info, 6, 2) == kMdMaxScore - 9 && md_item_inv_score(false, info, 6, 3) == kMdMaxScore);
    }
}

// ---- the worked cases of spm_hip.h ----
static stream worked(bool quals)
{
    stream S;
    auto add = [&](uint32_t read, uint32_t flag, int32_t pos, std::vector<uint32_t> cigar, std::vector<uint8_t> qual, int32_t ref_id = 0) {
        rec r;
        r.read = read;
        r.flag = flag;
        r.pos = pos;
        r.ref_id = ref_id;
        r.cigar = std::move(cigar);
        r.qual = std::move(qual);
        S.add(r);
    };
    auto ff = [](uint32_t n) { return std::vector<uint8_t>(n, 0xff); };
    add(0, 0, 100, {EQ(40)}, quals ? std::vector<uint8_t>(40, 10) : ff(40));
    add(1, 0, 100, {EQ(30)}, quals ? std::vector<uint8_t>(30, 30) : ff(30));
    add(2, 16, 111, {EQ(30)}, ff(30));
    add(3, 16, 101, {EQ(40)}, ff(40));
    add(4, 16, 100, {EQ(40)}, ff(40));
    add(5, 4, -1, {}, ff(20), -1);
    add(6, 97, 1000, {EQ(100)}, ff(100));
    add(7, 145, 1100, {EQ(100)}, ff(100));
    add(8, 97, 1000, {EQ(100)}, ff(100));
    add(9, 145, 1100, {EQ(100)}, ff(100));
    add(10, 97, 1000, {EQ(100)}, ff(100));
    add(11, 145, 1200, {EQ(100)}, ff(100));
    add(12, 73, 1000, {EQ(50)}, ff(50));
    add(13, 133, 1000, {}, ff(50));
    return S;
}

static void worked_cases()
{
    std::vector<uint8_t> dup;
    md_counts C;
    stream S = worked(false);
    EXPECT_TRUE(S.mark(10000, 15, dup, C));
    EXPECT_TRUE(dup == std::vector<uint8_t>({0, 1, 0, 1, 0, 0, 0, 0, 1, 1, 0, 0, 1, 0}));
    EXPECT_TRUE(C.n_pairs == 3 && C.n_fragments == 6 && C.n_dup_pairs == 1 && C.n_dup_fragments == 3 && C.n_dup_records == 5 &&
                C.n_fragments_beside_pairs == 1);
    EXPECT_TRUE(S.mark(1300, 15, dup, C) && !S.mark(1299, 15, dup, C));
    EXPECT_TRUE(dup == std::vector<uint8_t>(14, 7)); // a refused call leaves dup as it was found
    S = worked(true);
    EXPECT_TRUE(S.mark(10000, 15, dup, C) && dup[0] == 1 && dup[1] == 0);
    EXPECT_TRUE(S.mark(10000, 31, dup, C) && dup[0] == 0 && dup[1] == 1);
    // what the builder refuses
    stream T = worked(false);
    T.lines[4].read = 14;
    EXPECT_TRUE(!T.mark(10000, 15, dup, C));
    T = worked(false);
    T.lines[4].read = 3; // a second primary of read 3
    EXPECT_TRUE(!T.mark(10000, 15, dup, C));
    T = worked(false);
    T.lines[13].len += 1;
    EXPECT_TRUE(!T.mark(10000, 15, dup, C));
    T = worked(false);
    T.bytes[T.lines[3].offset + 20] = 41; // l_seq 41: qual leaves the record
    EXPECT_TRUE(!T.mark(10000, 15, dup, C));
    T = worked(false);
    T.bytes[T.lines[3].offset + 16] = 60; // the CIGAR leaves the record
    EXPECT_TRUE(!T.mark(10000, 15, dup, C));
    T = worked(false);
    T.bytes[T.lines[3].offset + 36 + 2] = (uint8_t)W(40, 4); // 40S
    EXPECT_TRUE(!T.mark(10000, 15, dup, C));
    T = worked(false);
    T.bytes[T.lines[5].offset + 36 + 2] = 0; // (read 5 has no CIGAR: this is its SEQ; unmapped records are not walked)
    EXPECT_TRUE(T.mark(10000, 15, dup, C));
    stream E;
    EXPECT_TRUE(E.mark(10000, 15, dup, C) && dup.empty() && C.n_pairs == 0);
}

// ---- random small record sets: serial builder, brute force, and the device's scheme ----
struct plan
{
    bool has_line = true, placed = false, paired = false, reverse = false;
    uint32_t u = 0, score = 0;
};

static void random_cases(uint32_t n_sets)
{
    std::mt19937 rng(20240607);
    const uint64_t ref_len = 64;
    const uint32_t pb = bam_pos_bits(ref_len);
    for (uint32_t set = 0; set < n_sets; ++set) {
        const uint32_t n_reads = 1 + rng() % 14;
        std::vector<plan> P(n_reads);
        std::vector<rec> recs;
        for (uint32_t r = 0; r < n_reads; ++r) {
            plan &p = P[r];
            p.placed = rng() % 8 != 0;
            p.paired = rng() % 3 != 0;
            p.reverse = rng() % 2;
            const uint32_t len = 1 + rng() % 4, pos = 10 + rng() % 4;
            rec x;
            x.read = r;
            x.flag = (p.paired ? 1u : 0u) | (p.reverse ? 16u : 0u) | (p.placed ? 0u : 4u) | (rng() % 2 ? 0x400u : 0u);
            x.pos = (int32_t)pos;
            x.cigar = p.placed ? std::vector<uint32_t>{EQ(len)} : std::vector<uint32_t>{};
            x.qual.resize(len);
            for (auto &q : x.qual)
                q = (uint8_t)(rng() % 3 == 0 ? 0xff : 14 + rng() % 3); // few distinct scores: ties are common
            x.name_len = 1 + rng() % 4;
            p.u = p.reverse ? pos + len - 1 : pos;
            for (uint8_t q : x.qual)
                p.score += (q >= 15 && q <= 93) ? q : 0;
            recs.push_back(x);
            if (rng() % 5 == 0) { // a secondary of the read, which never takes part
                rec y = x;
                y.flag |= rng() % 2 ? 0x100u : 0x800u;
                recs.push_back(y);
            }
        }
        std::shuffle(recs.begin(), recs.end(), rng);
        while (recs.size() < n_reads)
            recs.push_back(recs[0]); // (cannot be: every read has a line)
        stream S;
        for (const rec &x : recs)
            S.add(x);
        const uint64_t n = S.lines.size();
        std::vector<uint8_t> dup;
        md_counts C;
        EXPECT_TRUE(S.mark(ref_len, 15, dup, C));
        // brute force, from the plan
        auto pair_end = [&](uint32_t r) { return P[r].placed && P[r].paired && (r ^ 1) < n_reads && P[r ^ 1].placed && P[r ^ 1].paired; };
        auto code = [&](uint32_t r) { return (uint64_t)P[r].u << 1 | P[r].reverse; };
        auto pair_key = [&](uint32_t p) { return std::make_pair(std::min(code(2 * p), code(2 * p + 1)), std::max(code(2 * p), code(2 * p + 1))); };
        std::vector<uint8_t> want_read(n_reads, 0);
        md_counts B;
        for (uint32_t r = 0; r < n_reads; ++r) {
            if (!P[r].placed)
                continue;
            if (pair_end(r)) {
                const uint32_t p = r >> 1, sp = P[2 * p].score + P[2 * p + 1].score;
                for (uint32_t q = 0; 2 * q + 1 < n_reads; ++q) {
                    if (q == p || !pair_end(2 * q) || pair_key(q) != pair_key(p))
                        continue;
                    const uint32_t sq = P[2 * q].score + P[2 * q + 1].score;
                    want_read[r] |= sq > sp || (sq == sp && q < p);
                }
                B.n_pairs += r & 1;
                B.n_dup_pairs += (r & 1) && want_read[r];
            } else {
                bool beside = false;
                for (uint32_t q = 0; q < n_reads; ++q) {
                    if (q == r || !P[q].placed || code(q) != code(r))
                        continue;
                    if (pair_end(q))
                        beside = true;
                    else
                        want_read[r] |= P[q].score > P[r].score || (P[q].score == P[r].score && q < r);
                }
                want_read[r] |= beside;
                ++B.n_fragments;
                B.n_dup_fragments += want_read[r];
                B.n_fragments_beside_pairs += beside;
            }
        }
        bool same = true;
        for (uint64_t i = 0; i < n; ++i) {
            md_rec M;
            md_rec_read(S.bytes.data(), S.bytes.size(), S.lines[i].offset, S.lines[i].len, M);
            same = same && dup[i] == (md_is_primary(M.R.flag) && want_read[S.lines[i].read]);
        }
        EXPECT_TRUE(same);
        EXPECT_TRUE(C.n_pairs == B.n_pairs && C.n_dup_pairs == B.n_dup_pairs && C.n_fragments == B.n_fragments &&
                    C.n_dup_fragments == B.n_dup_fragments && C.n_fragments_beside_pairs == B.n_fragments_beside_pairs &&
                    C.n_dup_records == 2 * B.n_dup_pairs + B.n_dup_fragments);
        // the device's scheme over the same key functions: info by read (n slots), two stable sorts, the left neighbour
        std::vector<unsigned long long> info(n, 0);
        for (uint32_t r = 0; r < n_reads; ++r)
            if (P[r].placed)
                info[r] = md_info_pack(P[r].u, P[r].reverse, P[r].paired, md_score_clamp(P[r].score));
        std::vector<uint8_t> scheme(n, 0);
        for (bool pairs : {true, false}) {
            const uint64_t m = md_n_items(pairs, n);
            std::vector<uint32_t> idx(m);
            std::iota(idx.begin(), idx.end(), 0u);
            std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) {
                return md_item_inv_score(pairs, info.data(), n, a) < md_item_inv_score(pairs, info.data(), n, b);
            });
            std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) {
                return md_item_key(pairs, info.data(), n, a, pb) < md_item_key(pairs, info.data(), n, b, pb);
            });
            for (uint64_t j = 1; j < m; ++j) {
                if (!md_item_is_dup(pairs, md_item_key(pairs, info.data(), n, idx[j], pb), md_item_key(pairs, info.data(), n, idx[j - 1], pb), pb))
                    continue;
                if (pairs)
                    scheme[2 * idx[j]] = scheme[2 * idx[j] + 1] = 1;
                else
                    scheme[idx[j]] = 1;
            }
        }
        same = true;
        for (uint32_t r = 0; r < n_reads; ++r)
            same = same && scheme[r] == want_read[r];
        EXPECT_TRUE(same);
    }
}

int main()
{
    end_cases();
    score_cases();
    key_cases();
    worked_cases();
    random_cases(4000);
    std::printf("%d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}

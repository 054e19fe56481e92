// bam_index_core_cases.cpp -- the rule of the sorted BAM and its BAI index on the host (libspm_amd/csrc/bam_index_core.hpp):
// reg2bin of synthetic records against the record's bin field, the key order on hand-made ties, the end of a record for every
// CIGAR op, the virtual offset at a block border and at the stream's end, the two worked BAI cases of spm_hip.h byte for byte,
// records at both sides of (and across) every bin-level border through the serial builder, n_intv where end - 1 lies on a
// window border, and what the builder refuses.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../libspm_amd/csrc/bam_index_core.hpp"

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
#define EXPECT_STR(got, want)                                                                                          \
    do {                                                                                                               \
        ++checks;                                                                                                      \
        const std::string g_ = (got), w_ = (want);                                                                     \
        if (g_ != w_) {                                                                                                \
            ++failures;                                                                                                \
            std::printf("FAILED %s:%d:\n  got  %s\n  want %s\n", __FILE__, __LINE__, g_.c_str(), w_.c_str());          \
        }                                                                                                              \
    } while (0)

static std::string hex(const std::vector<uint8_t> &v)
{
    std::string s;
    char b[4];
    for (uint8_t c : v) {
        std::snprintf(b, sizeof(b), "%02x", c);
        s += b;
    }
    return s;
}
static std::string strip(const std::string &s)
{
    std::string o;
    for (char c : s)
        if (c != ' ' && c != '\n')
            o += c;
    return o;
}

// ---- a synthetic record stream: 36 fixed bytes, a one-letter name with its NUL, the CIGAR words ----
struct stream
{
    std::vector<uint8_t> bytes;
    std::vector<spm_sam_line> lines;
    void put32(uint32_t v)
    {
        for (int i = 0; i < 4; ++i)
            bytes.push_back((uint8_t)(v >> (8 * i)));
    }
    void add(int32_t ref_id, int32_t pos, uint32_t flag, const std::vector<uint32_t> &cigar, int bin = -1)
    {
        uint64_t span = 0;
        for (uint32_t w : cigar) {
            const uint32_t op = w & 15;
            span += (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) ? w >> 4 : 0;
        }
        if (flag & 4)
            span = 0;
        const uint32_t b = bin >= 0 ? (uint32_t)bin : jst_bam_bin(ref_id == 0 ? pos : -1, span);
        const uint32_t len = 36 + 2 + 4 * (uint32_t)cigar.size();
        spm_sam_line L{};
        L.offset = bytes.size();
        L.len = len;
        L.flag = (uint16_t)flag;
        lines.push_back(L);
        put32(len - 4);
        put32((uint32_t)ref_id);
        put32((uint32_t)pos);
        put32(2u | 0u << 8 | b << 16);
        put32((uint32_t)cigar.size() | flag << 16);
        put32(0);           // l_seq
        put32(0xFFFFFFFFu); // next_refID
        put32(0xFFFFFFFFu); // next_pos
        put32(0);           // tlen
        bytes.push_back('r');
        bytes.push_back(0);
        for (uint32_t w : cigar)
            put32(w);
    }
    bai_blocks stored(uint32_t D, uint64_t first) const
    {
        bai_blocks B;
        B.first = first;
        B.n_stream = bytes.size();
        B.n_blocks = bgzf_n_blocks(bytes.size(), D);
        B.D = D;
        return B;
    }
    bool build(uint32_t D, uint64_t first, std::vector<uint8_t> &out, bai_counts &C) const
    {
        return bai_build_serial(bytes.data(), bytes.size(), lines.data(), lines.size(), stored(D, first), out, C);
    }
};
static uint32_t M(uint32_t n) { return n << 4; }

// reg2bin from the specification's text, with a loop of its own
static uint32_t reg2bin_plain(int64_t beg, int64_t end)
{
    --end;
    const int shift[] = {14, 17, 20, 23, 26};
    const uint32_t first[] = {4681, 585, 73, 9, 1};
    for (int l = 0; l < 5; ++l)
        if (beg >> shift[l] == end >> shift[l])
            return first[l] + (uint32_t)(beg >> shift[l]);
    return 0;
}

// ---- a strict parse of the bytes the builder wrote ----
struct parsed
{
    struct bin
    {
        uint32_t id;
        std::vector<std::pair<uint64_t, uint64_t>> chunks;
    };
    std::vector<bin> bins;
    std::vector<uint64_t> ioffset;
    uint64_t n_no_coor = 0;
    bool ok = false;
};
static parsed parse(const std::vector<uint8_t> &v)
{
    parsed P;
    size_t at = 0;
    auto u32 = [&](uint32_t &x) {
        if (at + 4 > v.size())
            return false;
        x = bam_u32(v.data() + at);
        at += 4;
        return true;
    };
    auto u64 = [&](uint64_t &x) {
        uint32_t a, b;
        if (!u32(a) || !u32(b))
            return false;
        x = (uint64_t)b << 32 | a;
        return true;
    };
    uint32_t magic, n_ref, n_bin, n_intv;
    if (!u32(magic) || magic != 0x01494142u || !u32(n_ref) || n_ref != 1 || !u32(n_bin))
        return P;
    for (uint32_t b = 0; b < n_bin; ++b) {
        parsed::bin B;
        uint32_t n_chunk;
        if (!u32(B.id) || !u32(n_chunk) || n_chunk == 0)
            return P;
        for (uint32_t c = 0; c < n_chunk; ++c) {
            uint64_t x, y;
            if (!u64(x) || !u64(y))
                return P;
            B.chunks.push_back({x, y});
        }
        P.bins.push_back(B);
    }
    if (!u32(n_intv))
        return P;
    P.ioffset.resize(n_intv);
    for (uint64_t &x : P.ioffset)
        if (!u64(x))
            return P;
    P.ok = u64(P.n_no_coor) && at == v.size();
    return P;
}

// ---- reading a record, its end, its bin ----
static void record_cases()
{
    // every op: M I D N S H P = X; the reference symbols are those of M D N = X
    stream S;
    S.add(0, 1000, 0, {5u << 4 | 4, M(10), 3u << 4 | 1, 7u << 4 | 2, 100u << 4 | 3, 2u << 4 | 5, 1u << 4 | 6, 4u << 4 | 7, 2u << 4 | 8, 6u << 4 | 4});
    S.add(0, 2000, 4, {M(50)});      // unmapped beside its mate: end = pos + 1 whatever the CIGAR says
    S.add(0, 3000, 0, {});           // no CIGAR
    S.add(0, 4000, 0, {9u << 4 | 1}); // inside an insertion: span 0 counts as 1
    S.add(-1, -1, 4, {});
    const uint64_t want_end[] = {1000 + 10 + 7 + 100 + 4 + 2, 2001, 3001, 4001, 0};
    for (size_t i = 0; i < S.lines.size(); ++i) {
        bam_rec R;
        EXPECT_TRUE(bam_rec_read(S.bytes.data(), S.bytes.size(), S.lines[i].offset, S.lines[i].len, R));
        EXPECT_TRUE(bam_rec_end(S.bytes.data() + S.lines[i].offset, R) == want_end[i]);
        EXPECT_TRUE(R.flag == S.lines[i].flag && R.l_read_name == 2);
    }
    // at every byte alignment of the stream
    for (size_t shift = 1; shift < 4; ++shift) {
        std::vector<uint8_t> moved(shift, 0xEE);
        moved.insert(moved.end(), S.bytes.begin(), S.bytes.end());
        bam_rec R;
        EXPECT_TRUE(bam_rec_read(moved.data(), moved.size(), shift, S.lines[0].len, R) && R.pos == 1000 && R.n_cigar_op == 10);
        EXPECT_TRUE(bam_rec_end(moved.data() + shift, R) == want_end[0]);
    }
    // what a line may not be
    bam_rec R;
    const uint64_t n = S.bytes.size();
    EXPECT_TRUE(!bam_rec_read(S.bytes.data(), n, n - 10, 38, R));               // leaves the stream
    EXPECT_TRUE(!bam_rec_read(S.bytes.data(), n, n + 1, 0, R));
    EXPECT_TRUE(!bam_rec_read(S.bytes.data(), n, 0, 35, R));                    // shorter than the fixed part
    EXPECT_TRUE(!bam_rec_read(S.bytes.data(), n, 0, S.lines[0].len + 4, R));    // block_size is not len - 4
    std::vector<uint8_t> bad = S.bytes;
    bad[16] = 200;                                                              // n_cigar_op: the CIGAR leaves the record
    EXPECT_TRUE(!bam_rec_read(bad.data(), n, 0, S.lines[0].len, R));
    bad = S.bytes;
    bad[12] = 255;                                                              // l_read_name
    EXPECT_TRUE(!bam_rec_read(bad.data(), n, 0, S.lines[0].len, R));

    // reg2bin of synthetic records against the bin field, at both sides of and across every level border
    for (int level : {14, 17, 20, 23, 26})
        for (int64_t at = 1ll << level; at < (1ll << 29); at += (level < 20 ? 37ll : 5ll) << level) {
            for (int64_t beg : {at - 30, at - 1, at, at - 10}) {
                for (uint32_t len : {1u, 10u, 30u}) {
                    stream T;
                    T.add(0, (int32_t)beg, 0, {M(len)});
                    bam_rec Q;
                    EXPECT_TRUE(bam_rec_read(T.bytes.data(), T.bytes.size(), 0, T.lines[0].len, Q));
                    EXPECT_TRUE(Q.bin == reg2bin_plain(beg, beg + len) && Q.bin == jst_bam_reg2bin((int32_t)beg, (int32_t)(beg + len)));
                    EXPECT_TRUE(Q.bin < kBaiBins);
                }
            }
        }
}

// ---- the order ----
static void key_cases()
{
    auto key = [](int32_t ref_id, int32_t pos, uint32_t flag) {
        bam_rec R;
        R.ref_id = ref_id;
        R.pos = pos;
        R.flag = flag;
        return bam_key(R);
    };
    EXPECT_TRUE(key(0, 100, 0) < key(0, 100, 16));                   // one position: forward before reverse
    EXPECT_TRUE(key(0, 100, 0) == key(0, 100, 0x63));                // one position, one strand: a tie, the input order stays
    EXPECT_TRUE(key(0, 100, 16) < key(0, 101, 0));
    EXPECT_TRUE(key(0, 500, 0x85) == key(0, 500, 0x49));             // a placed unmapped mate sorts beside its mate ...
    EXPECT_TRUE(key(0, 500, 0x85) < key(0, 501, 0));
    EXPECT_TRUE(key(0, 0x7FFFFFFE, 16) < key(-1, -1, 4));            // ... and refID -1 goes to the end
    EXPECT_TRUE(key(0, 0, 0) < key(0, 0, 16) && key(-1, -1, 4) == key(-1, -1, 0x4D));
    // the packed key orders alike, in the bits ref_len needs
    EXPECT_TRUE(bam_pos_bits(1) == 1 && bam_pos_bits(2) == 2 && bam_pos_bits(1023) == 10 && bam_pos_bits(1024) == 11);
    EXPECT_TRUE(bam_pos_bits(0x7FFFFFFFull) == 31 && bam_sort_key_bits(31) == 33);
    for (uint64_t ref_len : {1ull, 12000ull, 1100000ull, 0x7FFFFFFFull}) {
        const uint32_t pb = bam_pos_bits(ref_len);
        const uint64_t keys[] = {key(0, 0, 0), key(0, 0, 16), key(0, (int32_t)(ref_len / 2), 0), key(0, (int32_t)ref_len - 1, 0),
                                 key(0, (int32_t)ref_len - 1, 16), key(-1, -1, 4)};
        for (size_t i = 0; i < 6; ++i) {
            EXPECT_TRUE(bam_key_packs(keys[i], pb) && bam_key_pack(keys[i], pb) >> bam_sort_key_bits(pb) == 0);
            for (size_t j = 0; j < 6; ++j)
                EXPECT_TRUE((keys[i] < keys[j]) == (bam_key_pack(keys[i], pb) < bam_key_pack(keys[j], pb)));
        }
        EXPECT_TRUE(ref_len == 0x7FFFFFFFull || !bam_key_packs(key(0, (int32_t)(1ull << pb), 0), pb)); // a position beyond the reference
    }
}

// ---- virtual offsets ----
static void voffset_cases()
{
    for (uint32_t D : {1u, 7u, 256u, 65280u}) {
        for (uint64_t n : {1ull * D, 3ull * D, 3ull * D + 1, 2ull * D + D / 2 + 1}) {
            bai_blocks B;
            B.first = 1000;
            B.n_stream = n;
            B.n_blocks = bgzf_n_blocks(n, D);
            B.D = D;
            std::vector<unsigned long long> table(B.n_blocks + 1);
            for (uint64_t b = 0; b <= B.n_blocks; ++b)
                table[b] = B.at(b);
            EXPECT_TRUE(table[0] == 1000 && table[B.n_blocks] == 1000 + bgzf_framed_size(n, D, false));
            bai_blocks T = B;
            T.table = table.data();
            for (uint64_t u : {0ull, D - 1ull, 1ull * D, n - 1ull, 1ull * n}) {
                if (u > n)
                    continue;
                EXPECT_TRUE(bai_voffset(B, u) == bai_voffset(T, u));
                EXPECT_TRUE(bai_voffset(B, u) == ((1000 + (u / D) * (D + 31ull)) << 16 | u % D) || (u == n && n % D == 0));
            }
            // u % D == 0: the first byte of the next block, not the byte behind the block before it
            EXPECT_TRUE(bai_voffset(B, D) == (1000ull + D + 31) << 16 || n == D);
            // the stream's end: a full last block ends at the EOF block's offset, a short one at its own length
            if (n % D == 0)
                EXPECT_TRUE(bai_voffset(B, n) == (1000 + bgzf_framed_size(n, D, false)) << 16);
            else
                EXPECT_TRUE(bai_voffset(B, n) == ((1000 + (n / D) * (D + 31ull)) << 16 | n % D));
        }
    }
}

// ---- the worked cases of spm_hip.h ----
static void worked_cases()
{
    std::vector<uint8_t> out;
    bai_counts C;
    stream none;
    EXPECT_TRUE(none.build(65280, 0, out, C));
    EXPECT_STR(hex(out), strip("42414901 01000000 00000000 00000000 0000000000000000"));
    EXPECT_TRUE(out.size() == 24 && C.n_bins == 0 && C.n_intv == 0 && C.n_no_coor == 0);

    stream S;
    S.add(0, 100, 0, {M(50)});
    S.add(0, 16380, 0, {M(10)});
    S.add(0, 16390, 16, {M(10)});
    S.add(-1, -1, 4, {});
    EXPECT_TRUE(S.bytes.size() == 164 && S.lines[3].offset == 126 && S.lines[3].len == 38);
    EXPECT_TRUE(S.build(100, 0, out, C));
    EXPECT_STR(hex(out), strip("42414901 01000000 04000000"
                               "49020000 01000000 2a00000000000000 5400000000000000"
                               "49120000 01000000 0000000000000000 2a00000000000000"
                               "4a120000 01000000 5400000000000000 1a00830000000000"
                               "4a920000 02000000 0000000000000000 1a00830000000000 0300000000000000 0000000000000000"
                               "02000000 0000000000000000 2a00000000000000"
                               "0100000000000000"));
    EXPECT_TRUE(out.size() == 152 && C.n_bins == 4 && C.n_chunks == 3 && C.n_intv == 2 && C.n_mapped == 3 && C.n_unmapped == 0 && C.n_no_coor == 1);
}

// ---- the builder at the bin-level borders ----
static void border_cases()
{
    for (uint32_t D : {1u, 7u, 256u, 65280u}) {
        stream S;
        std::vector<std::pair<int64_t, int64_t>> iv; // [beg, end) of the placed records, in order
        auto add = [&](int64_t beg, uint32_t len, uint32_t flag) {
            S.add(0, (int32_t)beg, flag, {M(len)});
            iv.push_back({beg, beg + (flag & 4 ? 1 : len)});
        };
        add(5, 20, 0);
        add(5, 20, 16);
        for (int level : {14, 17, 20, 23, 26}) {
            const int64_t at = 1ll << level;
            add(at - 40, 30, 0);  // before the border
            add(at - 40, 30, 0);  // an identical record: one chunk with the one before it
            add(at - 10, 20, 16); // across it
            add(at - 1, 1, 0);    // its last base
            add(at, 30, 0);       // behind it
            add(at, 30, 4);       // a placed unmapped mate
        }
        S.add(-1, -1, 4, {});
        S.add(-1, -1, 4, {});
        std::vector<uint8_t> out;
        bai_counts C;
        EXPECT_TRUE(S.build(D, 77, out, C));
        const parsed P = parse(out);
        EXPECT_TRUE(P.ok && P.n_no_coor == 2 && C.n_no_coor == 2 && C.n_unmapped == 5 && C.n_mapped == iv.size() - 5);
        EXPECT_TRUE(P.bins.size() == C.n_bins && P.bins.back().id == kBaiPseudoBin && P.bins.back().chunks.size() == 2);
        const bai_blocks B = S.stored(D, 77);
        // the bins ascend; every placed record lies in exactly one chunk of its reg2bin bin; chunks in file order
        size_t n_chunks = 0;
        for (size_t b = 0; b + 1 < P.bins.size(); ++b) {
            EXPECT_TRUE(b == 0 || P.bins[b - 1].id < P.bins[b].id);
            for (size_t c = 0; c < P.bins[b].chunks.size(); ++c) {
                EXPECT_TRUE(P.bins[b].chunks[c].first < P.bins[b].chunks[c].second);
                EXPECT_TRUE(c == 0 || P.bins[b].chunks[c - 1].second <= P.bins[b].chunks[c].first);
                ++n_chunks;
            }
        }
        EXPECT_TRUE(n_chunks == C.n_chunks);
        for (size_t i = 0; i < iv.size(); ++i) {
            const uint32_t bin = reg2bin_plain(iv[i].first, iv[i].second);
            const uint64_t vb = bai_voffset(B, S.lines[i].offset), ve = bai_voffset(B, S.lines[i].offset + S.lines[i].len);
            int found = 0;
            for (const auto &pb : P.bins)
                if (pb.id == bin)
                    for (const auto &ch : pb.chunks)
                        found += ch.first <= vb && ve <= ch.second;
            EXPECT_TRUE(found == 1);
        }
        // the two identical records in front of 2^17 (lines 8, 9) share a chunk: (begin of the first, end of the second); the record
        // across the border lies in another bin and ends the run, so the border's last base (line 11) is a chunk of its own
        for (const auto &pb : P.bins)
            if (pb.id == reg2bin_plain((1ll << 17) - 40, (1ll << 17) - 10))
                EXPECT_TRUE(pb.chunks.size() == 2 && pb.chunks[0].first == bai_voffset(B, S.lines[8].offset) &&
                            pb.chunks[0].second == bai_voffset(B, S.lines[10].offset) &&
                            pb.chunks[1].first == bai_voffset(B, S.lines[11].offset) && pb.chunks[1].second == bai_voffset(B, S.lines[12].offset));
        EXPECT_TRUE(P.bins.back().chunks[0].first == bai_voffset(B, 0) &&
                    P.bins.back().chunks[0].second == bai_voffset(B, S.lines[iv.size()].offset));
        EXPECT_TRUE(P.bins.back().chunks[1].first == C.n_mapped && P.bins.back().chunks[1].second == C.n_unmapped);
        // the linear index by its definition, window by window
        int64_t max_end = 0;
        for (const auto &x : iv)
            max_end = std::max(max_end, x.second);
        EXPECT_TRUE(P.ioffset.size() == (size_t)(((max_end - 1) >> 14) + 1) && P.ioffset.size() == 4097);
        uint64_t right = ~0ull;
        bool linear_ok = true;
        for (size_t w = P.ioffset.size(); w-- > 0;) {
            uint64_t m = ~0ull;
            for (size_t i = 0; i < iv.size(); ++i)
                if (iv[i].first < (int64_t)(w + 1) << 14 && iv[i].second > (int64_t)w << 14)
                    m = std::min(m, bai_voffset(B, S.lines[i].offset));
            right = m == ~0ull ? right : m; // an empty window: the next one to its right that is not
            linear_ok = linear_ok && P.ioffset[w] == right;
        }
        EXPECT_TRUE(linear_ok);
        // window 1 holds the record across 2^14 (line 4); windows 2 .. 6 are empty and take window 7's value (line 8)
        EXPECT_TRUE(P.ioffset[1] == bai_voffset(B, S.lines[4].offset) && P.ioffset[2] == P.ioffset[7] &&
                    P.ioffset[7] == bai_voffset(B, S.lines[8].offset));
    }
    // n_intv where end - 1 lies on a window border
    for (int64_t end : {16384ll, 16385ll, 16386ll, 32768ll, 32769ll}) {
        stream S;
        S.add(0, (int32_t)end - 3, 0, {M(3)});
        std::vector<uint8_t> out;
        bai_counts C;
        EXPECT_TRUE(S.build(65280, 0, out, C));
        EXPECT_TRUE(C.n_intv == (uint64_t)((end - 1) >> 14) + 1);
        EXPECT_TRUE(bai_n_intv(end) == C.n_intv);
    }
    EXPECT_TRUE(bai_n_intv(0) == 0 && bai_n_intv(1) == 1 && bai_n_intv(16384) == 1 && bai_n_intv(16385) == 2 && bai_n_intv(1ull << 29) == 32768);
}

// ---- what the builder refuses ----
static void refusal_cases()
{
    std::vector<uint8_t> out;
    bai_counts C;
    stream S;
    S.add(0, 100, 0, {M(10)});
    S.add(0, 100, 16, {M(10)});
    S.add(0, 200, 0, {M(10)});
    S.add(-1, -1, 4, {});
    EXPECT_TRUE(S.build(7, 0, out, C) && !out.empty());
    auto refused = [&](const stream &T, uint32_t D = 7) {
        std::vector<uint8_t> o(3, 1);
        bai_counts c;
        EXPECT_TRUE(!T.build(D, 0, o, c) && o.empty());
    };
    for (auto swap : {std::pair<int, int>{0, 1}, {1, 2}, {2, 3}}) { // out of coordinate order
        stream T;
        const int32_t pos[] = {100, 100, 200, -1};
        const uint32_t flag[] = {0, 16, 0, 4};
        int order[] = {0, 1, 2, 3};
        std::swap(order[swap.first], order[swap.second]);
        for (int i : order)
            T.add(i == 3 ? -1 : 0, pos[i], flag[i], i == 3 ? std::vector<uint32_t>{} : std::vector<uint32_t>{M(10)});
        refused(T);
    }
    stream T = S;
    T.lines[1].offset += 1; // does not follow the line before it
    refused(T);
    T = S;
    T.lines[3].len -= 1; // the last line does not end the stream
    refused(T);
    T = S;
    T.lines[2].len += 4; // block_size is not len - 4 (and the line before the last overlaps it)
    refused(T);
    T = S;
    T.bytes[T.lines[2].offset + 16] = 9; // a CIGAR that leaves the record
    refused(T);
    T = S;
    T.bytes[T.lines[2].offset + 4] = 1; // refID 1 of one reference
    refused(T);
    T = stream();
    T.add(0, -1, 0, {M(10)}); // placed at pos -1
    refused(T);
    T = stream();
    T.add(0, (1 << 29) - 5, 0, {M(6)}, 0); // ends beyond 2^29
    refused(T);
    T = stream();
    T.add(0, (1 << 29) - 5, 0, {M(5)});
    EXPECT_TRUE(T.build(7, 0, out, C) && C.n_intv == 32768);
    T = stream();
    T.add(0, 5, 0, {M(5)}, 37449); // a bin field beyond 37448
    refused(T);
    refused(S, 65281);
    bai_blocks B = S.stored(7, 0);
    B.D = 0;
    EXPECT_TRUE(!bai_build_serial(S.bytes.data(), S.bytes.size(), S.lines.data(), S.lines.size(), B, out, C));
    B = S.stored(7, 0);
    B.n_blocks += 1;
    EXPECT_TRUE(!bai_build_serial(S.bytes.data(), S.bytes.size(), S.lines.data(), S.lines.size(), B, out, C));
    B = S.stored(7, 0);
    EXPECT_TRUE(!bai_build_serial(S.bytes.data(), S.bytes.size(), S.lines.data(), 0, B, out, C)); // records without lines
}

int main()
{
    record_cases();
    key_cases();
    voffset_cases();
    worked_cases();
    border_cases();
    refusal_cases();
    std::printf("%d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}

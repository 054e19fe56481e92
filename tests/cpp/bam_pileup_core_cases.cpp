// bam_pileup_core_cases.cpp -- the rule of the pileup on the host (libspm_amd/csrc/bam_pileup_core.hpp): a SEQ nibble and a
// quality byte out of the dword that holds them against the byte walk, at all four alignments of the buffer, for names of 1..8
// bytes and odd and even l_seq, with the stream's last dword short; every CIGAR op in the worked table of spm_hip.h; what the
// serial builder refuses, with nothing written; on a few thousand random small sorted record sets the serial builder against a
// host emulation of the device's tile scheme -- pos[], end[], the running maximum, the two binary searches, the walk clipped to
// tile and region, every counter stored by exactly one tile -- with tiles of 4, 7 and 64 positions; and the sites of worked columns.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../libspm_amd/csrc/bam_pileup_core.hpp"

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

// ---- a synthetic record stream: 36 fixed bytes, a name with its NUL, the CIGAR words, the SEQ codes, the qualities ----
struct rec
{
    uint32_t flag = 0, mapq = 60;
    int32_t ref_id = 0, pos = 0;
    std::vector<uint32_t> cigar;
    std::vector<uint8_t> codes, qual; // l_seq of each
    uint32_t name_len = 1;
};
static uint32_t query_of(const std::vector<uint32_t> &cigar)
{
    uint32_t q = 0;
    for (uint32_t w : cigar)
        q += pu_op_query(w & 15u) ? w >> 4 : 0u;
    return q;
}
static rec make(int32_t pos, const std::vector<uint32_t> &cigar, const std::string &seq, uint32_t flag = 0)
{
    static const std::string letters = "=ACMGRSVTWYHKDBN";
    rec r;
    r.pos = pos;
    r.flag = flag;
    r.cigar = cigar;
    for (char ch : seq)
        r.codes.push_back((uint8_t)letters.find(ch));
    r.qual.assign(seq.size(), 0xff);
    return r;
}
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
        const uint32_t l_seq = (uint32_t)r.codes.size();
        const uint32_t len = 36 + r.name_len + 1 + 4 * (uint32_t)r.cigar.size() + (l_seq + 1) / 2 + l_seq;
        spm_sam_line L{};
        L.offset = bytes.size();
        L.len = len;
        L.read = (uint32_t)lines.size();
        L.flag = (uint16_t)r.flag;
        lines.push_back(L);
        put32(len - 4);
        put32((uint32_t)r.ref_id);
        put32((uint32_t)r.pos);
        put32((r.name_len + 1) | r.mapq << 8 | 4680u << 16);
        put32((uint32_t)r.cigar.size() | r.flag << 16);
        put32(l_seq);
        put32(~0u);
        put32(~0u);
        put32(0);
        bytes.insert(bytes.end(), r.name_len, (uint8_t)'r');
        bytes.push_back(0);
        for (uint32_t w : r.cigar)
            put32(w);
        for (uint32_t k = 0; k < l_seq; k += 2)
            bytes.push_back((uint8_t)(r.codes[k] << 4 | (k + 1 < l_seq ? r.codes[k + 1] : 0)));
        bytes.insert(bytes.end(), r.qual.begin(), r.qual.end());
    }
    bool pile(uint64_t ref_len, const pu_opts &O, std::vector<uint32_t> &counts) const
    {
        counts.assign(kPuPlanes * (O.end - O.begin) + 1, 7); // (+ 1: an empty region still has an address)
        return pileup_serial(bytes.data(), bytes.size(), lines.data(), lines.size(), ref_len, O, counts.data());
    }
};
static pu_opts region(uint64_t begin, uint64_t end)
{
    pu_opts O;
    O.begin = begin;
    O.end = end;
    O.exclude |= 4u;
    return O;
}

// ---- bytes out of dwords ----
static void extraction_cases()
{
    std::mt19937 rng(11);
    for (uint32_t mis = 0; mis < 4; ++mis)
        for (uint32_t name_len = 1; name_len <= 8; ++name_len)
            for (uint32_t l_seq = 30; l_seq <= 37; ++l_seq) {
                stream S;
                rec lead = make(3, {W(5, 0)}, "ACGTA"); // (the record under test does not start the stream)
                lead.name_len = 1 + (name_len + mis) % 3;
                S.add(lead);
                rec r;
                r.pos = 10;
                r.name_len = name_len;
                r.cigar = {W(l_seq, 0)};
                for (uint32_t k = 0; k < l_seq; ++k) {
                    r.codes.push_back((uint8_t)(rng() % 16));
                    r.qual.push_back((uint8_t)(rng() % 256));
                }
                S.add(r);
                // the stream at `mis` bytes behind a 4-byte border, ending with its last byte: the last dword may be short
                std::vector<uint32_t> aligned((S.bytes.size() + mis + 3) / 4 + 1);
                uint8_t *base = reinterpret_cast<uint8_t *>(aligned.data()) + mis;
                std::memcpy(base, S.bytes.data(), S.bytes.size());
                const uint64_t n_bytes = S.bytes.size();
                bool aligned_loads = true;
                auto load = [&](uint64_t a) {
                    aligned_loads = aligned_loads && (mis + a) % 4 == 0 && a < n_bytes;
                    uint32_t v = 0;
                    for (uint32_t i = 0; i < 4 && a + i < n_bytes; ++i)
                        v |= (uint32_t)base[a + i] << (8 * i);
                    return v;
                };
                pu_rec P;
                const uint64_t off = S.lines[1].offset;
                EXPECT_TRUE(pu_rec_read(base, n_bytes, off, S.lines[1].len, P));
                EXPECT_TRUE(P.M.l_seq == l_seq && P.mapq == 60 && P.seq_at == 36 + name_len + 1 + 4);
                bool same = true;
                for (uint32_t k = 0; k < l_seq; ++k) {
                    const uint32_t by_bytes = pu_seq_code(base[off + P.seq_at + k / 2], k);
                    const uint32_t by_dwords = pu_seq_code(pu_byte_by_dword(load, mis, off + P.seq_at + k / 2), k);
                    same = same && by_bytes == r.codes[k] && by_dwords == by_bytes;
                    same = same && pu_byte_by_dword(load, mis, off + P.M.qual_at + k) == r.qual[k];
                }
                EXPECT_TRUE(same);
                EXPECT_TRUE(aligned_loads);
                EXPECT_TRUE(off + P.M.qual_at + l_seq == n_bytes); // the last quality byte is the stream's last byte
            }
    EXPECT_TRUE(pu_base_plane(1) == kPuA && pu_base_plane(2) == kPuC && pu_base_plane(4) == kPuG && pu_base_plane(8) == kPuT);
    for (uint32_t code : {0u, 3u, 5u, 6u, 7u, 9u, 10u, 11u, 12u, 13u, 14u, 15u})
        EXPECT_TRUE(pu_base_plane(code) == kPuN);
    EXPECT_TRUE(pu_column_plane(1, 0, 1) == kPuLowq && pu_column_plane(1, 0, 0) == kPuA && pu_column_plane(2, 92, 93) == kPuLowq);
    EXPECT_TRUE(pu_column_plane(2, 93, 93) == kPuC && pu_column_plane(8, 255, 93) == kPuT && pu_column_plane(15, 255, 93) == kPuN);
}

// ---- the worked table of spm_hip.h ----
static std::vector<rec> worked_table()
{
    std::vector<rec> t = {make(10, {W(4, 0)}, "ACGT"),
                          make(10, {W(2, 7), W(1, 8), W(1, 7)}, "ACNT"),
                          make(11, {W(2, 0), W(2, 2), W(2, 0)}, "CGAA"),
                          make(12, {W(2, 0), W(3, 3), W(2, 0)}, "GTCC"),
                          make(12, {W(2, 1), W(3, 0)}, "TTGTA"),
                          make(12, {W(2, 4), W(1, 1), W(3, 0)}, "AATGTA"),
                          make(13, {W(2, 0), W(2, 1), W(2, 0)}, "TAGGAC"),
                          make(13, {W(3, 0), W(2, 4)}, "TAACC"),
                          make(14, {W(2, 5), W(3, 0), W(1, 6), W(2, 0), W(3, 5)}, "AACAC"),
                          make(15, {W(3, 0)}, "ACG"),
                          make(15, {W(3, 0)}, "AAA", 0x400),
                          make(-1, {}, "ACGTA", 4)};
    t[9].qual = {0, 20, 255};
    t[11].ref_id = -1;
    return t;
}
struct cell
{
    uint32_t plane, pos, n;
};
static void worked_cases()
{
    stream S;
    for (const rec &r : worked_table())
        S.add(r);
    const std::vector<cell> want = {{kPuA, 10, 2}, {kPuA, 14, 5}, {kPuA, 15, 5}, {kPuA, 16, 1}, {kPuA, 17, 1}, {kPuC, 11, 3}, {kPuC, 16, 3},
                                    {kPuC, 17, 1}, {kPuC, 18, 2}, {kPuG, 12, 5}, {kPuG, 17, 1}, {kPuT, 13, 7}, {kPuN, 12, 1}, {kPuDel, 13, 1},
                                    {kPuDel, 14, 1}, {kPuIns, 14, 1}};
    const uint64_t ref_len = 1000;
    auto expect = [&](const pu_opts &O, std::vector<cell> cells) {
        std::vector<uint32_t> got, table(kPuPlanes * (O.end - O.begin) + 1, 0);
        table.back() = 7;
        for (const cell &c : cells)
            if (c.pos >= O.begin && c.pos < O.end)
                table[c.plane * (O.end - O.begin) + (c.pos - O.begin)] += c.n;
        EXPECT_TRUE(S.pile(ref_len, O, got));
        EXPECT_TRUE(got == table);
    };
    expect(region(0, ref_len), want);
    expect(region(12, 15), want);
    expect(region(14, 14), want);
    pu_opts O = region(0, ref_len);
    O.min_baseq = 1;
    auto low = want;
    low.push_back({kPuLowq, 15, 1});
    low[2].n = 4;
    expect(O, low);
    O.min_baseq = 93;
    low.push_back({kPuLowq, 16, 1});
    low[6].n = 2;
    expect(O, low);
    O = region(0, ref_len);
    O.exclude = 4; // the duplicate takes part
    auto dup = want;
    for (uint32_t p : {15u, 16u, 17u})
        dup.push_back({kPuA, p, 1});
    expect(O, dup);
    O = region(0, ref_len);
    O.min_mapq = 61;
    expect(O, {});
    // ---- what the serial builder refuses: counts stay as they were found ----
    auto refused = [&](const std::vector<rec> &recs, uint64_t len) {
        stream B;
        for (const rec &r : recs)
            B.add(r);
        std::vector<uint32_t> got;
        EXPECT_TRUE(!B.pile(len, region(0, len), got));
        EXPECT_TRUE(std::count(got.begin(), got.end(), 7u) == (long)got.size());
    };
    auto t = worked_table();
    refused(t, 18); // records 3 and 8 end at 19
    std::swap(t[2], t[3]);
    refused(t, ref_len); // pos descends
    t = worked_table();
    std::swap(t[10], t[11]);
    refused(t, ref_len); // a placed record behind an unplaced one
    t = worked_table();
    t[3].cigar[1] = W(3, 9);
    refused(t, ref_len); // an op code above 8
    t = worked_table();
    t[4].codes.push_back(1);
    t[4].qual.push_back(0xff);
    refused(t, ref_len); // the CIGAR's query length is not l_seq
    t = worked_table();
    t[0].pos = -1;
    refused(t, ref_len);
    t = worked_table();
    t[9].ref_id = 1;
    refused(t, ref_len);
    t = worked_table();
    t[10].cigar[0] = W(3, 9); // ... but not of a record that does not take part
    t[10].pos = 990;
    t[10].cigar.push_back(W(50, 0));
    stream Q;
    for (const rec &r : t)
        Q.add(r);
    std::vector<uint32_t> got;
    EXPECT_TRUE(Q.pile(ref_len, region(0, ref_len), got));
}

// ---- the serial builder against the tile scheme ----
static std::vector<rec> random_set(std::mt19937 &rng, uint64_t ref_len)
{
    const uint32_t n = rng() % 14;
    std::vector<rec> recs;
    for (uint32_t i = 0; i < n; ++i) {
        rec r;
        r.name_len = 1 + rng() % 8;
        r.mapq = rng() % 4 ? 60 : rng() % 61;
        r.flag = (rng() % 8 == 0 ? 0x400u : 0u) | (rng() % 11 == 0 ? 0x100u : 0u) | (rng() % 13 == 0 ? 0x10u : 0u);
        const uint32_t items = rng() % 7;
        uint64_t span = 0;
        for (uint32_t k = 0; k < items; ++k) {
            const uint32_t op = rng() % 9, len = 1 + rng() % (op == 2 || op == 3 ? 40 : 9);
            r.cigar.push_back(W(len, op));
            span += pu_op_ref(op) ? len : 0;
        }
        span = span ? span : 1;
        if (span > ref_len)
            continue;
        r.pos = (int32_t)(rng() % (ref_len - span + 1));
        const uint32_t l_seq = query_of(r.cigar);
        for (uint32_t k = 0; k < l_seq; ++k) {
            r.codes.push_back((uint8_t)(rng() % 3 ? 1u << (rng() % 4) : rng() % 16));
            r.qual.push_back((uint8_t)(rng() % 5 ? rng() % 42 : 255));
        }
        recs.push_back(r);
    }
    std::stable_sort(recs.begin(), recs.end(), [](const rec &a, const rec &b) { return a.pos < b.pos; });
    for (uint32_t u = rng() % 3; u > 0; --u) { // unplaced records behind the placed ones
        rec r = make(-1, {}, "ACG", 4);
        r.ref_id = -1;
        recs.push_back(r);
    }
    return recs;
}

static bool tiles_emulated(const stream &S, uint64_t ref_len, const pu_opts &O, uint32_t T, std::vector<uint32_t> &out, uint64_t &visits)
{
    const uint64_t n = S.lines.size(), np = O.end - O.begin;
    const uint8_t *bytes = S.bytes.data();
    std::vector<uint32_t> pos(n), end(n), pmax(n);
    bam_rec prev;
    for (uint64_t i = 0; i < n; ++i) { // pu_records_kernel
        pu_rec P;
        uint64_t e = 0;
        const pu_status s = pu_rec_test(bytes, S.bytes.size(), S.lines[i].offset, S.lines[i].len, ref_len, O, P, e);
        if (s == kPuBad || (i && !pu_order_ok(prev, P.M.R)))
            return false;
        prev = P.M.R;
        pos[i] = pu_pos_key(P.M.R);
        end[i] = s == kPuTakes ? (uint32_t)e : 0u;
        pmax[i] = std::max(end[i], i ? pmax[i - 1] : 0u);
    }
    out.assign(kPuPlanes * np, 0xdeadbeefu);
    visits = 0;
    bool ok = true;
    for (uint64_t t0 = O.begin; t0 < O.end; t0 += T) { // pu_tiles_kernel, one tile after the other
        const uint64_t t1 = std::min<uint64_t>(t0 + T, O.end);
        std::vector<uint32_t> cnt(kPuPlanes * T, 0);
        const uint64_t i0 = pu_first_above(pmax.data(), n, t0), i1 = pu_first_at_or_behind(pos.data(), n, t1);
        for (uint64_t i = 0; i < n; ++i) // the bounds leave out no record that reaches into the tile
            ok = ok && ((i >= i0 && i < i1) || !(end[i] > t0 && pos[i] < t1));
        for (uint64_t i = i0; i < i1; ++i) {
            if (end[i] <= t0)
                continue;
            ++visits;
            pu_rec P;
            ok = ok && pu_rec_read(bytes, S.bytes.size(), S.lines[i].offset, S.lines[i].len, P);
            pu_walk(bytes + S.lines[i].offset, P, O.min_baseq, t0, t1, [&](uint32_t plane, uint64_t col) {
                ok = ok && col >= t0 && col < t1 && plane < kPuPlanes;
                if (col >= t0 && col < t1)
                    ++cnt[plane * T + (col - t0)];
            });
        }
        for (uint32_t p = 0; p < kPuPlanes; ++p)
            for (uint64_t x = 0; x < t1 - t0; ++x) {
                ok = ok && out[p * np + (t0 - O.begin) + x] == 0xdeadbeefu; // stored once
                out[p * np + (t0 - O.begin) + x] = cnt[p * T + x];
            }
    }
    return ok;
}

static void random_cases()
{
    std::mt19937 rng(2024);
    uint64_t sets = 0, evidence = 0, visits_all = 0;
    for (uint32_t round = 0; round < 3000; ++round) {
        const uint64_t ref_len = 20 + rng() % 300;
        stream S;
        for (const rec &r : random_set(rng, ref_len))
            S.add(r);
        pu_opts O = region(0, ref_len);
        if (rng() % 2) {
            O.begin = rng() % (ref_len + 1);
            O.end = O.begin + rng() % (ref_len - O.begin + 1);
        }
        O.min_baseq = rng() % 3 ? 0 : rng() % 45;
        O.min_mapq = rng() % 3 ? 0 : rng() % 62;
        O.exclude = (rng() % 2 ? kPuDefaultExclude : rng() % 2 ? 0x100u : 0u) | 4u;
        std::vector<uint32_t> want;
        const bool fine = S.pile(ref_len, O, want);
        EXPECT_TRUE(fine);
        want.pop_back();
        for (uint32_t T : {4u, 7u, 64u}) {
            std::vector<uint32_t> got;
            uint64_t visits = 0;
            EXPECT_TRUE(tiles_emulated(S, ref_len, O, T, got, visits));
            EXPECT_TRUE(got == want);
            visits_all += visits;
        }
        ++sets;
        for (uint32_t v : want)
            evidence += v;
    }
    EXPECT_TRUE(sets == 3000 && evidence > 30000 && visits_all > 3 * 3000);
}

// ---- sites ----
static void site_cases()
{
    struct col
    {
        uint8_t ref;
        uint32_t c[kPuPlanes];
    };
    const std::vector<col> cols = {{0, {3, 2, 0, 0, 0, 0, 0, 0}}, {0, {4, 1, 0, 0, 0, 0, 0, 0}}, {1, {0, 8, 0, 2, 0, 0, 0, 0}}, {1, {0, 9, 0, 2, 0, 0, 0, 0}},
                                   {0, {5, 0, 0, 0, 0, 0, 2, 0}}, {2, {0, 0, 0, 0, 0, 0, 0, 9}}, {3, {0, 0, 0, 2, 1, 3, 0, 0}}, {4, {2, 0, 0, 0, 4, 0, 0, 0}},
                                   {2, {0, 0, 0, 0, 0, 0, 0, 0}}, {3, {1, 1, 1, 1, 1, 1, 2, 1}}};
    const uint64_t n = cols.size(), begin = 40;
    std::vector<uint32_t> counts(kPuPlanes * n);
    std::vector<uint8_t> ref(begin + n + 3, 0);
    for (uint64_t k = 0; k < n; ++k) {
        ref[begin + k] = cols[k].ref;
        for (uint32_t p = 0; p < kPuPlanes; ++p)
            counts[p * n + k] = cols[k].c[p];
    }
    std::vector<spm_pileup_site> s;
    auto positions = [&](uint32_t min_depth, uint32_t min_alt, uint32_t permille) {
        pu_site_opts O;
        O.min_depth = min_depth;
        O.min_alt = min_alt;
        O.min_alt_permille = permille;
        pileup_sites_serial(counts.data(), begin, n, ref.data(), O, s);
        std::vector<uint32_t> at;
        for (const spm_pileup_site &x : s)
            at.push_back(x.pos);
        return at;
    };
    EXPECT_TRUE((positions(1, 2, 200) == std::vector<uint32_t>{40, 42, 44, 46, 47, 49}));
    EXPECT_TRUE(s[0].depth == 5 && s[0].alt == 2 && s[0].counts[0] == 3 && s[0].counts[1] == 2 && s[0].ref == 0);
    EXPECT_TRUE(s[3].depth == 6 && s[3].alt == 4 && s[3].counts[3] == 2 && s[3].ref == 3);
    EXPECT_TRUE(s[4].depth == 6 && s[4].alt == 2 && s[4].ref == 4 && s[5].alt == 7 && s[5].depth == 6);
    EXPECT_TRUE((positions(1, 1, 200) == std::vector<uint32_t>{40, 41, 42, 44, 46, 47, 49})); // alt == min_alt - 1 stays out at 2
    EXPECT_TRUE((positions(1, 2, 201) == std::vector<uint32_t>{40, 44, 46, 47, 49}));         // 1000 * 2 == 200 * 10 at 42
    EXPECT_TRUE((positions(1, 2, 181) == std::vector<uint32_t>{40, 42, 43, 44, 46, 47, 49}));  // 2000 >= 181 * 11 = 1991
    EXPECT_TRUE((positions(1, 2, 182) == std::vector<uint32_t>{40, 42, 44, 46, 47, 49}));      // 2000 < 2002
    EXPECT_TRUE(positions(0, 0, 0).size() == n && positions(1, 0, 0).size() == n - 2);
    EXPECT_TRUE((positions(1, 2, 1001) == std::vector<uint32_t>{49}) && positions(12, 0, 0).empty() && positions(11, 0, 0).size() == 1);
}

int main()
{
    extraction_cases();
    worked_cases();
    random_cases();
    site_cases();
    std::printf("%d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}

// jst_bam_core_cases.cpp -- the composition of a BAM record on the host (libspm_amd/csrc/jst_bam_core.hpp): reg2bin at the bin
// borders, the 4-bit codes in both cases of letter, for every kind of field and for whole records measured length == bytes
// written, the worked records of spm_hip.h byte for byte (and more: every kind of line the SAM rule knows), a merged M run of
// more than 64 words, what makes a record unwritable.  The fields of a line are set by hand here: how a line gets them is
// jst_sam_resolve's business and jst_sam_core_cases.cpp's.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../libspm_amd/csrc/jst_bam_core.hpp"

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

static const uint32_t EQ = SPM_CIGAR_EQ, MM = SPM_CIGAR_X, IN = SPM_CIGAR_INS, DE = SPM_CIGAR_DEL;
static uint32_t word(uint32_t len, uint32_t op) { return len << 4 | op; }

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
static std::string strip(std::string s) // the worked records are written with spaces between the fields
{
    std::string o;
    for (char c : s)
        if (c != ' ')
            o += c;
    return o;
}
static std::string times(const std::string &unit, int n)
{
    std::string s;
    for (int i = 0; i < n; ++i)
        s += unit;
    return s;
}

// ---- every sink operation: what the measuring sink adds is what the serial sink writes ----
template <class Op> static std::vector<uint8_t> through(Op &&op)
{
    jst_bam_measure M;
    op(M);
    std::vector<uint8_t> s(M.n + 4, 0xAA);
    jst_bam_serial W{s.data(), M.n, 0};
    op(W);
    EXPECT_TRUE(W.n == M.n);
    EXPECT_TRUE(s[M.n] == 0xAA && s[M.n + 3] == 0xAA); // nothing beyond what was measured
    std::vector<uint8_t> t(M.n + 1, 0xAA);             // a sink with too little room counts on and writes nothing beyond its cap
    jst_bam_serial C{t.data(), M.n / 2, 0};
    op(C);
    bool clean = C.n == M.n;
    for (uint64_t i = M.n / 2; i < t.size(); ++i)
        clean = clean && t[i] == 0xAA;
    EXPECT_TRUE(clean);
    s.resize(M.n);
    return s;
}

static void bin_cases()
{
    EXPECT_TRUE(jst_bam_reg2bin(-1, 0) == 4680);
    EXPECT_TRUE(jst_bam_reg2bin(0, 1) == 4681);
    EXPECT_TRUE(jst_bam_reg2bin(0, 16384) == 4681);
    EXPECT_TRUE(jst_bam_reg2bin(0, 16385) == 585);
    EXPECT_TRUE(jst_bam_reg2bin(16383, 16385) == 585);
    // [2^26 - 1, 2^26 + 1) lies across the border of the two 2^26 bins 1 and 2: the specification's function answers 0
    EXPECT_TRUE(jst_bam_reg2bin((1 << 26) - 1, (1 << 26) + 1) == 0);
    EXPECT_TRUE(jst_bam_reg2bin((1 << 23) - 1, (1 << 23) + 1) == 1); // inside bin 1, across two 2^23 bins
    EXPECT_TRUE(jst_bam_reg2bin((1 << 26), (1 << 26) + (1 << 23) + 1) == 2);
    EXPECT_TRUE(jst_bam_reg2bin((1 << 29) - 1, (1 << 29) + 1) == 0);
    EXPECT_TRUE(jst_bam_reg2bin(16384, 16385) == 4682 && jst_bam_reg2bin((1 << 29) - 1, 1 << 29) == 4681 + 32767);
    EXPECT_TRUE(jst_bam_reg2bin(0, 1 << 17) == 585 && jst_bam_reg2bin(0, (1 << 17) + 1) == 73 && jst_bam_reg2bin(0, (1 << 20) + 1) == 9);
    // the bin of a record: a span of 0 counts as 1, no position is 4680
    EXPECT_TRUE(jst_bam_bin(-1, 0) == 4680 && jst_bam_bin(-1, 30) == 4680);
    EXPECT_TRUE(jst_bam_bin(0, 0) == 4681 && jst_bam_bin(0, 1) == 4681 && jst_bam_bin(16383, 0) == 4681 && jst_bam_bin(16383, 2) == 585);
    EXPECT_TRUE(jst_bam_bin(99, 32) == 4681 && jst_bam_bin(0x7FFFFFFE, 0) == 4681 + 131071 && jst_bam_bin(0x7FFFFFFE, 5) == 4681 + 131071);
}

static void nibble_cases()
{
    const char *letters = "=ACMGRSVTWYHKDBN";
    for (int i = 0; i < 16; ++i) {
        EXPECT_TRUE(jst_bam_nibble(letters[i]) == i);
        if (letters[i] != '=')
            EXPECT_TRUE(jst_bam_nibble((char)(letters[i] + 32)) == i);
    }
    for (char c : {'U', 'u', 'X', 'x', '*', '.', '-', ' ', '\0', '1', 'E', '@', '`', '{', '\x7f', (char)0xC1})
        EXPECT_TRUE(jst_bam_nibble(c) == 15);
    uint8_t codes[256];
    jst_bam_rank_codes("acgTn", 5, codes);
    EXPECT_TRUE(codes[0] == 1 && codes[1] == 2 && codes[2] == 4 && codes[3] == 8 && codes[4] == 15);
    for (int r = 5; r < 256; ++r)
        EXPECT_TRUE(codes[r] == 15); // a rank >= sigma
    jst_bam_rank_codes("AC", 2, codes);
    EXPECT_TRUE(codes[2] == 15 && codes[3] == 15);
}

static void field_cases()
{
    uint8_t codes[256];
    jst_bam_rank_codes("ACGT", 4, codes);
    const uint32_t w[9] = {0x04030201u, 0x08070605u, 0xFFFFFFFFu, 0, 0x80000000u, 1, 2, 3, 0xA0B0C0D0u};
    EXPECT_STR(hex(through([&](auto &k) { k.fixed(w); })), "0102030405060708ffffffff00000000000000800100000002000000" "03000000d0c0b0a0");
    EXPECT_STR(hex(through([&](auto &k) { k.bytes("r1/x", 4); })), "72312f78");
    EXPECT_STR(hex(through([&](auto &k) { k.bytes("", 0); })), "");
    for (uint64_t v : {0ull, 7ull, 10ull, 4294967295ull, 18446744073709551615ull}) {
        const std::string want = std::to_string(v);
        const std::vector<uint8_t> got = through([&](auto &k) { k.num(v); });
        EXPECT_STR(std::string(got.begin(), got.end()), want);
    }
    EXPECT_STR(hex(through([&](auto &k) { k.fill(0xff, 3); })), "ffffff");
    EXPECT_STR(hex(through([&](auto &k) { k.fill(0, 1); })), "00");
    EXPECT_STR(hex(through([&](auto &k) { k.fill(0xff, 0); })), "");
    // SEQ: two per byte, the first in the high nibble; odd lengths leave the last low nibble 0
    const uint8_t ranks[7] = {0, 1, 2, 3, 9, 0, 3};
    EXPECT_STR(hex(through([&](auto &k) { k.seq(ranks, 7, codes); })), "1248f180");
    EXPECT_STR(hex(through([&](auto &k) { k.seq(ranks, 6, codes); })), "1248f1");
    EXPECT_STR(hex(through([&](auto &k) { k.seq(ranks, 1, codes); })), "10");
    EXPECT_STR(hex(through([&](auto &k) { k.seq(ranks, 0, codes); })), "");
    // tags: seven bytes whatever the value
    EXPECT_STR(hex(through([&](auto &k) { k.tag(jst_bam_tag_head('N', 'M', 'i'), (uint32_t)-1); })), "4e4d69ffffffff");
    EXPECT_STR(hex(through([&](auto &k) { k.tag(jst_bam_tag_head('X', '0', 'I'), 0xFFFFFFFFu); })), "583049ffffffff");
    EXPECT_STR(hex(through([&](auto &k) { k.tag(jst_bam_tag_head('X', 'N', 'I'), 2); })), "584e4902000000");
    // CIGAR: the words as they are; with merge every maximal run of = / X one M
    const std::vector<uint32_t> t = {word(20, EQ), word(1, MM), word(11, EQ), word(2, IN), word(3, EQ), word(1, DE), word(4, MM)};
    EXPECT_STR(hex(through([&](auto &k) { k.cigar(t.data(), 7, false); })), "47010000" "18000000" "b7000000" "21000000" "37000000" "12000000" "48000000");
    EXPECT_STR(hex(through([&](auto &k) { k.cigar(t.data(), 7, true); })), "00020000" "21000000" "30000000" "12000000" "40000000");
    EXPECT_STR(hex(through([&](auto &k) { k.cigar(t.data(), 3, true); })), "00020000");
    EXPECT_STR(hex(through([&](auto &k) { k.cigar(t.data() + 3, 1, true); })), "21000000");
    EXPECT_TRUE(jst_bam_item_word(32, word(11, EQ), true) == 0x200 && jst_bam_item_word(11, word(11, EQ), false) == word(11, EQ));
    EXPECT_TRUE(jst_bam_item_word(2, word(2, IN), true) == word(2, IN));
    // a merged run of more than 64 words: 35 X between 36 =, one M of 150; then an I, then another run
    std::vector<uint32_t> lng;
    for (int i = 0; i < 35; ++i) {
        lng.push_back(word(i == 0 ? 2 : 3, EQ));
        lng.push_back(word(1, MM));
    }
    lng.push_back(word(11, EQ));
    uint64_t q, r;
    jst_sam_cigar_spans(lng.data(), (uint32_t)lng.size(), q, r);
    EXPECT_TRUE(lng.size() == 71 && q == 150 && r == 150);
    EXPECT_STR(hex(through([&](auto &k) { k.cigar(lng.data(), 71, true); })), "60090000");
    EXPECT_TRUE(through([&](auto &k) { k.cigar(lng.data(), 71, false); }).size() == 4 * 71);
    lng.push_back(word(1, IN));
    lng.push_back(word(7, MM));
    EXPECT_STR(hex(through([&](auto &k) { k.cigar(lng.data(), 73, true); })), "60090000" "11000000" "70000000");
}

// ---- whole records ----
struct line
{
    jst_sam_src S;
    jst_sam_fields F;
    std::vector<uint32_t> words;
    std::vector<uint8_t> seq;
    uint8_t codes[256];
    std::string names;
    std::vector<uint64_t> name_off;

    line()
    {
        S.symbols = "ACGT";
        S.sigma = 4;
        S.rname = "chr";
        S.rname_len = 3;
        jst_bam_rank_codes("ACGT", 4, codes);
    }
    // a mapped line at POS with the given words; the SEQ is `letter` rank repeated over the query length
    void mapped(uint8_t kind, uint64_t name, uint32_t flag, uint64_t pos, uint32_t mapq, std::vector<uint32_t> w, uint8_t rank = 0)
    {
        words = std::move(w);
        uint64_t q, r;
        jst_sam_cigar_spans(words.data(), (uint32_t)words.size(), q, r);
        seq.assign(q, rank);
        F.kind = kind;
        F.name = name;
        F.flag = flag;
        F.pos = pos;
        F.mapq = mapq;
        F.words = words.data();
        F.n_words = (uint32_t)words.size();
        F.seq = kind == SPM_SAM_SECONDARY_LINE ? nullptr : seq.data();
        F.m = (uint32_t)q;
        F.rname = true;
    }
    void mate(uint64_t pnext, int32_t tlen)
    {
        F.rnext = true;
        F.pnext = pnext;
        F.tlen = tlen;
    }
    std::vector<uint8_t> record(uint64_t ref_len = 1 << 20, bool *ok = nullptr)
    {
        jst_bam_shape H;
        const bool good = jst_bam_shape_of(S, F, ref_len, H);
        if (ok)
            *ok = good;
        else
            EXPECT_TRUE(good);
        jst_bam_measure M;
        jst_bam_compose(S, F, H, codes, 0, M);
        std::vector<uint8_t> out = through([&](auto &k) { jst_bam_compose(S, F, H, codes, (uint32_t)M.n - 4, k); });
        EXPECT_TRUE(out.size() == M.n && out.size() >= 38);
        return out;
    }
};

static void record_cases()
{
    const std::string NM1 = "4e4d69 01000000", XH0 = "584869 00000000";
    // 1. single-end reverse, 20= 1X 11= at [99,131), read 7, MAPQ 40, 2 haplotypes, n_best 1, n_next 1
    for (bool merge : {false, true}) {
        line L;
        L.S.flags = merge ? SPM_SAM_CIGAR_M : 0;
        L.mapped(SPM_SAM_LOCUS, 7, 16, 100, 40, {word(20, EQ), word(1, MM), word(11, EQ)});
        L.F.nm = 1;
        L.F.xn = 2;
        L.F.x0 = 1;
        L.F.x1 = 1;
        const std::string tail = times("11", 16) + times("ff", 32) + NM1 + XH0 + "584e49 02000000" "583049 01000000" "583149 01000000";
        if (!merge)
            EXPECT_STR(hex(L.record()), strip("81000000 00000000 63000000 02 28 4912 0300 1000 20000000 ffffffff ffffffff 00000000 3700"
                                              "47010000 18000000 b7000000" + tail));
        else
            EXPECT_STR(hex(L.record()), strip("79000000 00000000 63000000 02 28 4912 0100 1000 20000000 ffffffff ffffffff 00000000 3700"
                                              "00020000" + tail));
        EXPECT_TRUE(L.record().size() == (merge ? 125u : 133u));
    }
    // 2. a proper pair: mate 1 forward at [1000,1030), mate 2 at POS 1171, TLEN 200, MAPQ 60; and its mate with TLEN -200
    {
        line L;
        L.mapped(SPM_SAM_LOCUS, 0, 99, 1001, 60, {word(30, EQ)}, 1);
        L.mate(1171, 200);
        L.F.xn = 1;
        L.F.x0 = 1;
        EXPECT_STR(hex(L.record()), strip("76000000 00000000 e8030000 02 3c 4912 0100 6300 1e000000 00000000 92040000 c8000000 3000 e7010000" +
                                          times("22", 15) + times("ff", 30) +
                                          "4e4d69 00000000 584869 00000000 584e49 01000000 583049 01000000 583149 00000000"));
        L.mapped(SPM_SAM_LOCUS, 0, 147, 1171, 60, {word(30, EQ)}, 3);
        L.mate(1001, -200);
        const std::string r = hex(L.record());
        EXPECT_STR(r.substr(8, 64), strip("00000000 92040000 02 3c 4912 0100 9300 1e000000 00000000 e8030000 38ffffff"));
    }
    // 3. a rescued mate: NM 4, XR 1, the anchor's counts (n_best 2: MAPQ 3)
    {
        line L;
        L.mapped(SPM_SAM_RESCUE, 12, 147, 1171, 3, {word(10, EQ), word(4, MM), word(16, EQ)}, 2);
        L.mate(1001, -200);
        L.F.nm = 4;
        L.F.x0 = 2;
        const std::string r = hex(L.record());
        EXPECT_STR(r.substr(0, 78), strip("78000000 00000000 92040000 03 03 4912 0300 9300 1e000000 00000000 e8030000 38ffffff 313200"));
        EXPECT_STR(r.substr(r.size() - 56), strip("4e4d69 04000000 585269 01000000 583049 02000000 583149 00000000"));
        EXPECT_TRUE(r.size() == 2 * (4 + 0x78));
    }
    // 4. an unmapped mate beside a mapped one at POS 501: RNAME and POS are the mate's, no CIGAR, no tags; SEQ ACG (odd l_seq)
    {
        line L;
        L.seq = {0, 1, 2};
        L.F.kind = SPM_SAM_UNMAPPED;
        L.F.name = 0;
        L.F.flag = 133;
        L.F.pos = 501;
        L.F.seq = L.seq.data();
        L.F.m = 3;
        L.F.rname = true;
        L.mate(501, 0);
        EXPECT_STR(hex(L.record()), strip("27000000 00000000 f4010000 02 00 4912 0000 8500 03000000 00000000 f4010000 00000000 3000 1240 ffffff"));
        // ... and an unmapped single-end read: no reference, no position, bin 4680
        L.F.flag = 4;
        L.F.pos = 0;
        L.F.rname = L.F.rnext = false;
        L.F.pnext = 0;
        EXPECT_STR(hex(L.record()), strip("27000000 ffffffff ffffffff 02 00 4812 0000 0400 03000000 ffffffff ffffffff 00000000 3000 1240 ffffff"));
    }
    // 5. a secondary: no SEQ, no QUAL, MAPQ 255, no X0 / X1
    {
        line L;
        L.mapped(SPM_SAM_SECONDARY_LINE, 0, 401, 7001, 255, {word(4, EQ)});
        L.mate(1001, 0);
        L.F.xn = 1;
        EXPECT_STR(hex(L.record()), strip("3b000000 00000000 581b0000 02 ff 4912 0100 9101 00000000 00000000 e8030000 00000000 3000 47000000"
                                          "4e4d69 00000000 584869 00000000 584e49 01000000"));
    }
    // 6. a locus inside an insertion: span 0, end = pos + 1; a name of the caller's
    {
        line L;
        L.names = "ab*cd";
        L.name_off = {0, 2, 5};
        L.S.names = L.names.data();
        L.S.name_off = L.name_off.data();
        L.mapped(SPM_SAM_LOCUS, 1, 0, 16384, 60, {word(3, IN)}, 3);
        L.F.nm = 3;
        L.F.xh = -2;
        L.F.xn = 0xFFFFFFFFu;
        EXPECT_STR(hex(L.record()), strip("50000000 00000000 ff3f0000 04 3c 4912 0100 0000 03000000 ffffffff ffffffff 00000000 2a636400 31000000 8880 ffffff"
                                          "4e4d69 03000000 584869 feffffff 584e49 ffffffff 583049 00000000 583149 00000000"));
        L.F.pos = 16385; // ... one further: the next bin
        EXPECT_STR(hex(L.record()).substr(24, 8), strip("04 3c 4a12"));
    }
    // whole records of every shape: measured == written (through() checks), and block_size is the length less 4
    for (uint32_t n_words : {1u, 2u, 63u, 64u, 65u, 200u})
        for (bool merge : {false, true}) {
            line L;
            L.S.flags = merge ? SPM_SAM_CIGAR_M : 0;
            std::vector<uint32_t> w;
            for (uint32_t i = 0; i < n_words; ++i)
                w.push_back(word(1 + i % 3, i % 5 == 4 ? DE : i % 7 == 6 ? IN : i % 2 ? MM : EQ));
            L.mapped(SPM_SAM_LOCUS, 123456, 0, 5, 9, w, 2);
            const std::vector<uint8_t> r = L.record();
            uint32_t bs;
            memcpy(&bs, r.data(), 4);
            EXPECT_TRUE(bs + 4 == r.size() && r[12] == 7);
            const uint32_t items = r[16] | r[17] << 8;
            EXPECT_TRUE(merge ? items < n_words || n_words <= 1 : items == n_words);
        }
}

static void predicate_cases()
{
    EXPECT_TRUE(jst_bam_items_ok(0) && jst_bam_items_ok(65535) && !jst_bam_items_ok(65536));
    EXPECT_TRUE(!jst_bam_run_ok(0) && jst_bam_run_ok(1) && jst_bam_run_ok((1u << 28) - 1) && !jst_bam_run_ok(1u << 28));
    EXPECT_TRUE(jst_bam_end_ok(100, 100) && !jst_bam_end_ok(101, 100) && jst_bam_end_ok(0, 1));
    bool ok = false;
    {   // an end beyond the reference: [99, 131) in a reference of 130
        line L;
        L.mapped(SPM_SAM_LOCUS, 0, 0, 100, 60, {word(32, EQ)});
        L.record(131, &ok);
        EXPECT_TRUE(ok);
        L.record(130, &ok);
        EXPECT_TRUE(!ok);
    }
    {   // a word of length 0
        line L;
        L.mapped(SPM_SAM_LOCUS, 0, 0, 100, 60, {word(5, EQ), word(0, DE), word(5, EQ)});
        L.record(1 << 20, &ok);
        EXPECT_TRUE(!ok);
    }
    {   // a merged run above 2^28 - 1: each word fits, their sum does not
        line L;
        L.S.flags = SPM_SAM_CIGAR_M;
        std::vector<uint32_t> w = {word((1u << 28) - 1, EQ), word(1, MM)};
        L.F.kind = SPM_SAM_SECONDARY_LINE; // (no SEQ of 2^28 symbols)
        L.F.pos = 1;
        L.F.words = w.data();
        L.F.n_words = 2;
        L.F.rname = true;
        jst_bam_shape H;
        EXPECT_TRUE(!jst_bam_shape_of(L.S, L.F, 0x7FFFFFFF, H));
        L.S.flags = 0;
        EXPECT_TRUE(jst_bam_shape_of(L.S, L.F, 0x7FFFFFFF, H) && H.n_items == 2);
    }
    {   // more than 65535 items; merged they are one
        line L;
        std::vector<uint32_t> w;
        for (uint32_t i = 0; i < 65536; ++i)
            w.push_back(word(1, i & 1 ? MM : EQ));
        L.F.kind = SPM_SAM_SECONDARY_LINE;
        L.F.pos = 1;
        L.F.words = w.data();
        L.F.n_words = 65536;
        L.F.rname = true;
        jst_bam_shape H;
        EXPECT_TRUE(!jst_bam_shape_of(L.S, L.F, 0x7FFFFFFF, H));
        L.F.n_words = 65535;
        EXPECT_TRUE(jst_bam_shape_of(L.S, L.F, 0x7FFFFFFF, H) && H.n_items == 65535);
        L.F.n_words = 65536;
        L.S.flags = SPM_SAM_CIGAR_M;
        EXPECT_TRUE(jst_bam_shape_of(L.S, L.F, 0x7FFFFFFF, H) && H.n_items == 1 && H.bin == jst_bam_reg2bin(0, 65536));
    }
}

int main()
{
    bin_cases();
    nibble_cases();
    field_cases();
    record_cases();
    predicate_cases();
    std::printf("%d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}

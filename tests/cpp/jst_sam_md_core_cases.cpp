// jst_sam_md_core_cases.cpp -- the two kinds of field that spm_sam_extras adds, on the host (libspm_amd/csrc/jst_sam_core.hpp and
// jst_bam_core.hpp): the MD string of a transcript and the base qualities of a line.  The worked cases of spm_hip.h; measured
// length == bytes written on random transcripts, in the text's sinks and in the record's; the serial sink with a buffer one byte
// short; counts at the digit borders; a transcript that starts and ends in X, D directly followed by X, = I =, a rank >= sigma;
// the qualities forward and back to front at the lengths around a wave; whole lines and records with both.  The expected strings
// come from a rendering written here (md_by_columns) that compares the read with the reference column by column.
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
static const char *const SYM = "ACGT";

static std::vector<uint8_t> ranks(const std::string &s)
{
    std::vector<uint8_t> r;
    for (char c : s)
        r.push_back(c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 4);
    return r;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) // 0 .. n - 1
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)((rng_state >> 20) % n);
}

// the MD of a transcript through both sinks of the text: the measured length is the written length
static std::string md_of(const std::vector<uint32_t> &w, const std::vector<uint8_t> &ref, uint64_t begin, uint32_t sigma = 4)
{
    jst_sam_measure M;
    M.md(w.data(), (uint32_t)w.size(), ref.data() + begin, SYM, sigma);
    std::vector<char> buf(M.n + 8, '#');
    jst_sam_serial S{buf.data(), M.n, 0};
    S.md(w.data(), (uint32_t)w.size(), ref.data() + begin, SYM, sigma);
    EXPECT_TRUE(S.n == M.n);
    for (size_t i = M.n; i < buf.size(); ++i)
        EXPECT_TRUE(buf[i] == '#');
    return std::string(buf.data(), M.n);
}

// the read a transcript describes over ref at begin: = copies, X takes another rank, I takes rank 1
static std::vector<uint8_t> read_of(const std::vector<uint32_t> &w, const std::vector<uint8_t> &ref, uint64_t begin)
{
    std::vector<uint8_t> read;
    uint64_t r = begin;
    for (uint32_t x : w) {
        const uint32_t op = x & 15u, n = x >> 4;
        for (uint32_t i = 0; i < n; ++i) {
            if (op == EQ)
                read.push_back(ref[r + i]);
            else if (op == MM)
                read.push_back((uint8_t)((ref[r + i] + 1 + rnd(3)) & 3));
            else if (op == IN)
                read.push_back(1);
        }
        r += op == IN ? 0 : n;
    }
    return read;
}

// MD by comparing columns, as a consumer without the = / X of the transcript would
static std::string md_by_columns(const std::vector<uint32_t> &w, const std::vector<uint8_t> &read, const std::vector<uint8_t> &ref,
                                 uint64_t begin)
{
    std::string out;
    uint64_t c = 0, q = 0, r = begin;
    auto letter = [&](uint64_t at) { return ref[at] < 4 ? SYM[ref[at]] : 'N'; };
    for (uint32_t x : w) {
        const uint32_t op = x & 15u, n = x >> 4;
        if (op == IN) {
            q += n;
        } else if (op == DE) {
            out += std::to_string(c) + "^";
            for (uint32_t i = 0; i < n; ++i)
                out += letter(r + i);
            c = 0;
            r += n;
        } else {
            for (uint32_t i = 0; i < n; ++i) {
                if (read[q + i] == ref[r + i]) {
                    ++c;
                } else {
                    out += std::to_string(c) + letter(r + i);
                    c = 0;
                }
            }
            q += n;
            r += n;
        }
    }
    return out + std::to_string(c);
}

static bool md_grammar(const std::string &s) // [0-9]+(([A-Z]|\^[A-Z]+)[0-9]+)*
{
    size_t i = 0;
    auto digits = [&] {
        const size_t at = i;
        while (i < s.size() && s[i] >= '0' && s[i] <= '9')
            ++i;
        return i > at;
    };
    auto upper = [&] { return i < s.size() && s[i] >= 'A' && s[i] <= 'Z'; };
    if (!digits())
        return false;
    while (i < s.size()) {
        if (s[i] == '^') {
            ++i;
            if (!upper())
                return false;
            while (upper())
                ++i;
        } else if (upper()) {
            ++i;
        } else {
            return false;
        }
        if (!digits())
            return false;
    }
    return true;
}

static void worked_cases()
{
    const std::vector<uint8_t> lead = ranks("GATTACA");
    struct one
    {
        std::vector<uint32_t> w;
        std::string stretch, md;
    };
    const one cases[] = {
        {{word(20, EQ), word(1, MM), word(11, EQ)}, std::string(20, 'T') + "G" + std::string(11, 'T'), "20G11"},
        {{word(5, EQ), word(2, MM), word(3, EQ), word(2, DE), word(1, MM), word(4, EQ)}, "TTTTTACTTTGTATTTT", "5A0C3^GT0A4"},
        {{word(3, MM)}, "ACG", "0A0C0G0"},
        {{word(4, EQ), word(2, IN), word(4, EQ)}, "CCCCCCCC", "8"},
        {{word(30, IN)}, "", "0"},
    };
    for (const one &c : cases) {
        std::vector<uint8_t> ref = lead, tail = ranks(c.stretch + "CAT");
        ref.insert(ref.end(), tail.begin(), tail.end());
        EXPECT_STR(md_of(c.w, ref, 7), c.md);
        EXPECT_STR(md_by_columns(c.w, read_of(c.w, ref, 7), ref, 7), c.md);
        EXPECT_TRUE(jst_sam_md_agrees(c.w.data(), (uint32_t)c.w.size(), ref.data() + 7, read_of(c.w, ref, 7).data()));
    }
    EXPECT_STR(md_of({}, lead, 3), "0"); // no words at all
}

static void named_shapes()
{
    const std::vector<uint8_t> ref = ranks("ACGTTGCAACGTACGTNACGTACGTACGTACGTACGTACGTACGT");
    EXPECT_STR(md_of({word(1, MM), word(3, EQ), word(1, MM)}, ref, 0), "0A3T0");      // starts and ends in X
    EXPECT_STR(md_of({word(2, EQ), word(2, DE), word(1, MM), word(2, EQ)}, ref, 0), "2^GT0T2"); // D directly followed by X
    EXPECT_STR(md_of({word(2, EQ), word(1, MM), word(2, DE), word(2, EQ)}, ref, 0), "2G0^TT2"); // X directly followed by D
    EXPECT_STR(md_of({word(3, EQ), word(5, IN), word(4, EQ)}, ref, 1), "7");          // = I =: the insertion does not end the run
    EXPECT_STR(md_of({word(3, EQ), word(1, IN), word(1, MM), word(1, IN), word(2, EQ)}, ref, 0), "3T2");
    EXPECT_STR(md_of({word(2, EQ), word(1, MM), word(1, EQ)}, ref, 14), "2N1");       // a rank >= sigma
    EXPECT_STR(md_of({word(1, DE), word(2, EQ)}, ref, 16), "0^N2");
    EXPECT_STR(md_of({word(2, EQ), word(1, MM), word(1, EQ)}, ranks("ACGT"), 0, 2), "2N1"); // sigma 2: G is beyond it
    EXPECT_STR(md_of({word(2, EQ), word(0, MM), word(0, DE), word(2, EQ)}, ref, 0), "4");  // words of length 0 print nothing
    // counts at the digit borders
    std::vector<uint8_t> longref(260, 2);
    for (uint32_t n : {9u, 10u, 99u, 100u}) {
        const std::string d = std::to_string(n);
        EXPECT_STR(md_of({word(n, EQ), word(1, MM), word(n, EQ)}, longref, 0), d + "G" + d);
        EXPECT_STR(md_of({word(n, EQ), word(2, DE), word(n, EQ)}, longref, 0), d + "^GG" + d);
        EXPECT_TRUE(jst_sam_md_word_len(n, word(1, MM)) == d.size() + 1 && jst_sam_md_word_len(n, word(3, MM)) == d.size() + 5);
        EXPECT_TRUE(jst_sam_md_word_len(n, word(70, DE)) == d.size() + 71);
    }
    // a wrong reference: an X column whose rank is the read's
    const std::vector<uint32_t> w = {word(2, EQ), word(2, MM), word(2, EQ)};
    std::vector<uint8_t> read = read_of(w, ref, 4);
    EXPECT_TRUE(jst_sam_md_agrees(w.data(), 3, ref.data() + 4, read.data()));
    read[3] = ref[4 + 3];
    EXPECT_TRUE(!jst_sam_md_agrees(w.data(), 3, ref.data() + 4, read.data()));
}

static void short_buffer()
{
    const std::vector<uint8_t> ref = ranks("ACGTACGTAC");
    const std::vector<uint32_t> w = {word(3, EQ), word(1, MM), word(2, DE), word(2, EQ)};
    const std::string want = "3A0^CG2";
    EXPECT_STR(md_of(w, ref, 1), want);
    for (size_t cap = 0; cap <= want.size(); ++cap) { // the serial sink counts on beyond cap and writes nothing there
        std::vector<char> buf(want.size() + 4, '#');
        jst_sam_serial S{buf.data(), cap, 0};
        S.md(w.data(), (uint32_t)w.size(), ref.data() + 1, SYM, 4);
        EXPECT_TRUE(S.n == want.size());
        EXPECT_STR(std::string(buf.data(), cap), want.substr(0, cap));
        for (size_t i = cap; i < buf.size(); ++i)
            EXPECT_TRUE(buf[i] == '#');
    }
}

static void random_transcripts()
{
    std::vector<uint8_t> ref(4000);
    for (uint8_t &x : ref)
        x = (uint8_t)(rnd(100) == 0 ? 4 : rnd(4));
    for (int it = 0; it < 4000; ++it) {
        std::vector<uint32_t> w;
        uint32_t last = 0, span = 0;
        const uint32_t n_words = 1 + rnd(it % 10 == 0 ? 150 : 12); // some of more than 64 words
        for (uint32_t i = 0; i < n_words; ++i) {
            uint32_t op;
            do {
                const uint32_t pick = rnd(5);
                op = pick < 2 ? EQ : pick == 2 ? MM : pick == 3 ? IN : DE;
            } while (op == last);
            last = op;
            const uint32_t n = op == EQ ? 1 + rnd(120) : op == DE ? 1 + rnd(80) : 1 + rnd(3);
            if (op != IN && span + n > 3000)
                break;
            span += op == IN ? 0 : n;
            w.push_back(word(n, op));
        }
        if (w.empty())
            w.push_back(word(3, IN));
        const uint64_t begin = rnd((uint32_t)ref.size() - span);
        const std::vector<uint8_t> read = read_of(w, ref, begin);
        const std::string md = md_of(w, ref, begin);
        EXPECT_STR(md, md_by_columns(w, read, ref, begin));
        EXPECT_TRUE(md_grammar(md));
        EXPECT_TRUE(jst_sam_md_agrees(w.data(), (uint32_t)w.size(), ref.data() + begin, read.data()));
        // the record's sinks: MD Z, the same string, NUL
        jst_bam_measure BM;
        BM.md(w.data(), (uint32_t)w.size(), ref.data() + begin, SYM, 4);
        EXPECT_TRUE(BM.n == md.size() + 4);
        std::vector<uint8_t> buf(BM.n + 4, 0xAA);
        jst_bam_serial BS{buf.data(), BM.n, 0};
        BS.md(w.data(), (uint32_t)w.size(), ref.data() + begin, SYM, 4);
        EXPECT_TRUE(BS.n == BM.n && buf[BM.n] == 0xAA);
        EXPECT_STR(std::string(buf.begin(), buf.begin() + (long)BM.n), std::string("MDZ") + md + std::string(1, '\0'));
    }
}

static void qualities()
{
    for (uint32_t m : {1u, 2u, 63u, 64u, 65u, 130u, 200u}) {
        std::vector<uint8_t> q(m);
        for (uint32_t i = 0; i < m; ++i)
            q[i] = (uint8_t)((i * 7 + m) % 94);
        q[0] = 0;
        q[m - 1] = 93;
        for (bool reverse : {false, true}) {
            for (uint8_t add : {(uint8_t)0, (uint8_t)33}) {
                jst_sam_measure M;
                M.qual(q.data(), m, reverse, add);
                EXPECT_TRUE(M.n == m);
                std::vector<char> buf(m + 2, '#');
                jst_sam_serial S{buf.data(), m, 0};
                S.qual(q.data(), m, reverse, add);
                EXPECT_TRUE(S.n == m && buf[m] == '#');
                std::vector<uint8_t> raw(m + 2, 0xAA);
                jst_bam_serial B{raw.data(), m, 0};
                B.qual(q.data(), m, reverse, add);
                EXPECT_TRUE(B.n == m && raw[m] == 0xAA);
                for (uint32_t i = 0; i < m; ++i) {
                    const uint8_t want = (uint8_t)(q[reverse ? m - 1 - i : i] + add);
                    EXPECT_TRUE((uint8_t)buf[i] == want && raw[i] == want);
                    EXPECT_TRUE(jst_sam_qual_byte(q.data(), m, reverse, add, i) == want);
                }
            }
        }
    }
    const uint8_t nine = 9; // a one-base read with Phred 9 prints '*': the specification's own ambiguity, left as it is
    EXPECT_TRUE(jst_sam_qual_byte(&nine, 1, false, 33, 0) == '*');
}

// a whole line and a whole record with both fields, by hand: worked case 1 of the header on a reference that has the G
static void whole_line_and_record()
{
    std::vector<uint8_t> ref(200, 3), needle(32, 3), qual(32);
    ref[99 + 20] = 2;
    needle[20] = 0;
    for (uint32_t i = 0; i < 32; ++i)
        qual[i] = (uint8_t)(i + 2);
    const uint32_t w[3] = {word(20, EQ), word(1, MM), word(11, EQ)};
    jst_sam_src S;
    S.symbols = SYM;
    S.sigma = 4;
    S.rname = "chr";
    S.rname_len = 3;
    jst_sam_fields F;
    F.name = 7;
    F.pos = 100;
    F.words = w;
    F.n_words = 3;
    F.seq = needle.data();
    F.m = 32;
    F.flag = 16;
    F.mapq = 40;
    F.nm = 1;
    F.xn = 2;
    F.x0 = F.x1 = 1;
    F.kind = SPM_SAM_LOCUS;
    F.rname = true;
    auto text = [&] {
        jst_sam_measure M;
        jst_sam_compose(S, F, M);
        std::vector<char> buf(M.n);
        jst_sam_serial W{buf.data(), M.n, 0};
        jst_sam_compose(S, F, W);
        EXPECT_TRUE(W.n == M.n);
        return std::string(buf.begin(), buf.end());
    };
    const std::string seq = std::string(20, 'T') + "A" + std::string(11, 'T');
    EXPECT_STR(text(), "7\t16\tchr\t100\t40\t20=1X11=\t*\t0\t0\t" + seq + "\t*\tNM:i:1\tXH:i:0\tXN:i:2\tX0:i:1\tX1:i:1\n");
    F.qual = qual.data();
    F.qual_reverse = true;
    F.md_ref = ref.data() + 99;
    std::string q;
    for (uint32_t i = 0; i < 32; ++i)
        q += (char)(33 + qual[31 - i]);
    EXPECT_STR(text(), "7\t16\tchr\t100\t40\t20=1X11=\t*\t0\t0\t" + seq + "\t" + q + "\tNM:i:1\tMD:Z:20G11\tXH:i:0\tXN:i:2\tX0:i:1\tX1:i:1\n");
    S.flags = SPM_SAM_CIGAR_M; // the MD string does not change with M
    EXPECT_STR(text(), "7\t16\tchr\t100\t40\t32M\t*\t0\t0\t" + seq + "\t" + q + "\tNM:i:1\tMD:Z:20G11\tXH:i:0\tXN:i:2\tX0:i:1\tX1:i:1\n");
    S.flags = 0;
    // the record: 133 bytes without, + 9 (4d 44 5a "20G11" 00) with MD, the qualities in place of ff
    uint8_t codes[256];
    jst_bam_rank_codes(SYM, 4, codes);
    jst_bam_shape H;
    EXPECT_TRUE(jst_bam_shape_of(S, F, 200, H));
    jst_bam_measure M;
    jst_bam_compose(S, F, H, codes, 0, M);
    EXPECT_TRUE(M.n == 133 + 9);
    std::vector<uint8_t> rec(M.n);
    jst_bam_serial W{rec.data(), M.n, 0};
    jst_bam_compose(S, F, H, codes, (uint32_t)M.n - 4, W);
    EXPECT_TRUE(W.n == M.n);
    const size_t at_qual = 36 + 2 + 12 + 16;
    for (uint32_t i = 0; i < 32; ++i)
        EXPECT_TRUE(rec[at_qual + i] == qual[31 - i]);
    EXPECT_TRUE(std::memcmp(rec.data() + at_qual + 32, "NMi\1\0\0\0MDZ20G11\0XHi", 19) == 0);
    EXPECT_TRUE(rec[0] == 142 - 4 && rec[1] == 0);
    // a secondary line: SEQ and QUAL "*", MD stays
    F.kind = SPM_SAM_SECONDARY_LINE;
    F.seq = nullptr;
    F.qual = nullptr;
    F.flag = 272;
    F.mapq = 255;
    EXPECT_STR(text(), "7\t272\tchr\t100\t255\t20=1X11=\t*\t0\t0\t*\t*\tNM:i:1\tMD:Z:20G11\tXH:i:0\tXN:i:2\n");
}

int main()
{
    worked_cases();
    named_shapes();
    short_buffer();
    random_transcripts();
    qualities();
    whole_line_and_record();
    std::printf("%d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
